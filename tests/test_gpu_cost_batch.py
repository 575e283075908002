"""GPU: the batched running cost (socp_cost_batch[_dev] / _blocks, capi.Context.cost_batch) against tests/cost_reference.py --
the definition restated in numpy -- driven (1) by the CPU oracle's right-hand side and Hamiltonian and (2) by the context's own
socp_eval_batch.  Outputs live in sentinel-filled buffers followed by 64 guard words and are compared WHOLE on uint64 views
(the conventions of test_gpu_trace_batch.py).  Exact flavour: bit equality.  Throughput flavour: e_new = max|batch_fast -
batch_exact| within 2 e_old + 16 ulp of the largest magnitude, e_old = max|composition_fast - batch_exact| (the helper driven by
the fast context's eval_batch) -- the factor 2 because both are independent contractions of the same arithmetic -- and, at
1e4 steps, the project's bar for that flavour, 1e-8 max(1, |cost|), against the exact flavour's batch.
The figures the tests print belong in profiles/cost_gpu_tests.txt (not measured yet)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GODDARD_X0_STATE, GODDARD_PSTAR, GODDARD_TF, goddard_c1_problem
from cost_reference import reference_cost_lanes
from test_gpu_trace_batch import model_sw, perturbed, read_obstacles

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = np.uint64(0x7FF8DEADBEEF0001)            # a NaN no kernel produces
GUARD = 64
EPS = 2.0 ** -52
DP = C.POINTER(C.c_double)


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def sentinel(size):
    return np.full(size + GUARD, SENT, dtype=np.uint64).view(np.float64)


# ---- running the entry points on guarded buffers: each returns the three WHOLE buffers as uint64 ---------------------------

def run_host(ctx, Z, total=True, xend=True):
    B, M, s = len(Z), ctx.M, ctx.s
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    cost, tot, xe = sentinel(B * M), sentinel(B), sentinel(B * M * s)
    ctx._chk(ctx.L.socp_cost_batch(ctx.h, B, Z.ctypes.data_as(DP), cost.ctypes.data_as(DP), tot.ctypes.data_as(DP) if total else None,
                                   xe.ctypes.data_as(DP) if xend else None))
    return cost.view(np.uint64), tot.view(np.uint64), xe.view(np.uint64)


def run_dev(ctx, Z, total=True, xend=True, blocks=None):
    import torch
    B, M, s = len(Z), ctx.M, ctx.s
    dZ = torch.from_numpy(np.ascontiguousarray(Z, dtype=np.float64)).cuda()
    dC, dT, dX = (torch.from_numpy(sentinel(k)).cuda() for k in (B * M, B, B * M * s))
    keep = []
    if blocks is not None:
        ptrs = []
        for a in blocks:
            if a is None:
                ptrs.append(None)
            else:
                keep.append(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda())
                ptrs.append(keep[-1].data_ptr())
        ctx._chk(ctx.L.socp_problem_set_blocks_dev(ctx.h, ptrs[0], blocks[0].shape[1] if blocks[0] is not None else 0, ptrs[1], ptrs[2]))
    torch.cuda.synchronize()
    try:
        ctx.cost_batch_dev(B, dZ.data_ptr(), dC.data_ptr(), dT.data_ptr() if total else None, dX.data_ptr() if xend else None)
        ctx.synchronize()
        torch.cuda.synchronize()
    finally:
        if blocks is not None:
            ctx.L.socp_problem_set_blocks_dev(ctx.h, None, 0, None, None)
    return tuple(t.cpu().numpy().view(np.uint64) for t in (dC, dT, dX))


def check_whole(got, want, what=""):
    """got: the three whole buffers; want: (cost[B][M], total[B] or None, xend[B][M][s] or None) -- None: nothing may be written."""
    for name, g, w in zip(("cost", "total", "xend"), got, want):
        if w is None:
            assert np.all(g == SENT), "%s: %s was written although its pointer was NULL" % (what, name)
            continue
        w = u64(w).ravel()
        assert np.all(g[w.size:] == SENT), "%s: guard words behind %s were written" % (what, name)
        bad = np.argwhere(g[:w.size] != w)
        assert len(bad) == 0, (what, name, "first differing flat indices:", bad[:5].ravel().tolist(),
                               g[:w.size].view(np.float64)[bad[:5].ravel()], w.view(np.float64)[bad[:5].ravel()])


def left_to_right(cost):
    total = cost[:, 0].copy()
    for i in range(1, cost.shape[1]):
        total = total + cost[:, i]
    return total


# ---- the lanes of a batch and the two references -------------------------------------------------------------------------

def lanes_of(ctx, mode_t, Z):
    """(t1, t2, sw, X_start) of every lane T = b M + i, as the kernel's prologue forms them."""
    s, M = ctx.s, len(mode_t) - 1
    t1, t2, sw, X0 = [], [], [], []
    for z in Z:
        tl = ctx.timeline(z)
        pair = model_sw(ctx, mode_t, tl, False)
        for i in range(M):
            t1.append(tl[i]), t2.append(tl[i + 1]), sw.append(pair), X0.append(z[s * i:s * (i + 1)])
    return np.array(t1), np.array(t2), np.array(sw), np.array(X0)


def reference_oracle(o, ctx, mode_t, Z, N):
    t1, t2, sw, X0 = lanes_of(ctx, mode_t, Z)

    def rhs(idx, t, Y):
        out = np.empty_like(Y)
        for k, lane in enumerate(idx):
            o.set_switching(sw[lane])
            out[k] = o.rhs(float(t[k]), Y[k])
        return out

    def ham(idx, t, Y):
        out = np.empty(len(idx))
        for k, lane in enumerate(idx):
            o.set_switching(sw[lane])
            out[k] = o.hamiltonian(float(t[k]), Y[k])[0]
        return out
    q, Xe = reference_cost_lanes(rhs, ham, ctx.dim, t1, t2, X0, N)
    cost = q.reshape(len(Z), -1)
    return cost, left_to_right(cost), Xe.reshape(len(Z), cost.shape[1], ctx.s)


def reference_composition(ctx, mode_t, Z, N):
    """The same helper driven by the context's own evaluation kernels, each lane with its sw pair."""
    from socp_amd import capi
    t1, t2, sw, X0 = lanes_of(ctx, mode_t, Z)
    rhs = lambda idx, t, Y: ctx.eval_batch(capi.EVAL_RHS, t, Y, sw=sw[idx])                    # noqa: E731
    ham = lambda idx, t, Y: ctx.eval_batch(capi.EVAL_HAMILTONIAN, t, Y, sw=sw[idx])[:, 0]      # noqa: E731
    q, Xe = reference_cost_lanes(rhs, ham, ctx.dim, t1, t2, X0, N)
    cost = q.reshape(len(Z), -1)
    return cost, left_to_right(cost), Xe.reshape(len(Z), cost.shape[1], ctx.s)


def segment_ends(ctx, mode_t, Z):
    t1, t2, sw, X0 = lanes_of(ctx, mode_t, Z)
    return ctx.integrate_batch(t1, t2, X0, sw=sw).reshape(len(Z), len(mode_t) - 1, ctx.s)


# ---- layouts (test 1; reused by the throughput-flavour and the error tests) --------------------------------------------------

def set_variant(ctx, variant):
    from socp_amd import capi
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)


def goddard_nodes(o, M, tf=GODDARD_TF):
    Xi = np.concatenate([GODDARD_X0_STATE, GODDARD_PSTAR])
    time = np.array([i * tf / M for i in range(M + 1)])
    X = np.zeros((M + 1, 14))
    X[0, :7] = GODDARD_X0_STATE
    X[M, 0] = 1.01
    nodes = np.stack([Xi] + [o.traj(0.0, Xi, time[i]) for i in range(1, M)])
    return time, X, nodes


def costates_perturbed(nodes, B, eps, seed):
    """B copies of the node states, the costates of every node scaled by 1 + eps xi, xi uniform(-1, 1): the form of the project's
    synthetic starts (conftest.goddard_costate_batch)."""
    rng = np.random.default_rng(seed)
    Z = np.tile(nodes, (B, 1, 1))
    Z[:, :, 7:] *= 1.0 + eps * rng.uniform(-1.0, 1.0, size=(B, nodes.shape[0], 7))
    return Z.reshape(B, -1)


def build_goddard_fixed(B, M, N, variant="exact", tf=0.03, eps=1e-2):
    """Fixed tf, M segments with interpolated (CONTINUOUS) interior times; mu2 = 1.  Nodes on the nominal trajectory, costates
    perturbed.  The horizon is short on purpose: at 10 steps the flight over [0, 0.03] amplifies a rounding of its start state
    about 400 times (measured with the CPU oracle), over the whole flight [0, GODDARD_TF] 4e7 times and, with the position perturbed
    by 1 %, without bound (the state ends at 1e26) -- an input on which two flavours cannot be compared."""
    from socp_amd import capi
    from oracle.oracle import Oracle, MODEL_GODDARD
    o = Oracle(MODEL_GODDARD, step_nbr=N)
    o.set_param("mu2", 1.0)
    ctx = capi.Context(capi.MODEL_GODDARD)
    set_variant(ctx, variant)
    ctx.set_param("mu2", 1.0)
    ctx.set_step_number(N)
    o.set_params(ctx.get_params())
    time, X, nodes = goddard_nodes(o, M, tf)
    mode_t = [capi.FIXED] + [capi.CONTINUOUS] * (M - 1) + [capi.FIXED]
    mode_x = np.zeros((M + 1, 7), dtype=np.int32)
    mode_x[1:M] = capi.CONTINUOUS
    mode_x[M, 3:7] = capi.FREE
    assert ctx.problem_set(mode_t, mode_x, time, X) == 14 * M
    return ctx, o, mode_t, costates_perturbed(nodes, B, eps, seed=B + M), N


def build_goddard_c1(B=5, N=10, variant="exact"):
    from socp_amd import capi
    from oracle.oracle import Oracle, MODEL_GODDARD
    o = Oracle(MODEL_GODDARD, step_nbr=N)
    o.set_param("mu2", 1.0)
    ctx = capi.Context(capi.MODEL_GODDARD)
    set_variant(ctx, variant)
    ctx.set_param("mu2", 1.0)
    ctx.set_step_number(N)
    o.set_params(ctx.get_params())
    prob, _ = goddard_c1_problem(o)
    assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == 85
    # around the CONVERGED unknowns of that problem (tests/golden, drag continuation at KD = 310): the test's own initial guess
    # (costates 0.1) sends the state to 1e6 .. 1e38 within a segment, an input on which two flavours cannot be compared
    z = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "goddard_flow.json")))["goddard_N10_M6"][1]["z"])
    assert len(z) == 85
    return ctx, o, list(prob.mode_t), perturbed(z, B, rel=0.002, seed=7), N


def build_goddard_n87(B=3, N=10, variant="exact"):
    """testGoddard's last stage: mu2 = 0, two FREE interior times (the switching times come from z) and free tf; the general
    control law with its bang, singular and off arcs."""
    from socp_amd import capi
    from oracle.oracle import Oracle, MODEL_GODDARD
    z = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "goddard_flow.json")))["goddard_N10_M6"][3]["z"])
    assert len(z) == 87
    o = Oracle(MODEL_GODDARD, step_nbr=N)
    ctx = capi.Context(capi.MODEL_GODDARD)
    set_variant(ctx, variant)
    ctx.set_param("mu2", 0.0)
    ctx.set_param("singularControl", -1.0)
    ctx.set_step_number(N)
    o.set_params(ctx.get_params())
    M = 6
    mode_t = [capi.FIXED, capi.CONTINUOUS, capi.FREE, capi.CONTINUOUS, capi.FREE, capi.CONTINUOUS, capi.FREE]
    mode_x = np.full((M + 1, 7), capi.CONTINUOUS, dtype=np.int32)
    mode_x[0] = capi.FIXED
    mode_x[M] = 0
    mode_x[M, 3:7] = capi.FREE
    X = np.zeros((M + 1, 14))
    X[0, :7] = GODDARD_X0_STATE
    X[M, 0] = 1.01
    assert ctx.problem_set(mode_t, mode_x, np.linspace(0.0, z[-1], M + 1), X) == 87
    return ctx, o, mode_t, perturbed(z, B, rel=0.002, seed=11), N


def build_dint_wp(B=4, N=10, variant="exact"):
    """testDoubleIntegrator_WP's layout: M = 2, every time after the first FREE (one of them interior)."""
    from socp_amd import capi
    from oracle.oracle import Oracle, MODEL_DINT
    o = Oracle(MODEL_DINT, step_nbr=N)
    ctx = capi.Context(capi.MODEL_DOUBLE_INTEGRATOR)
    set_variant(ctx, variant)
    ctx.set_step_number(N)
    o.set_params(ctx.get_params())
    M = 2
    mode_t = [capi.FIXED] + [capi.FREE] * M
    mode_x = np.zeros((M + 1, 6), dtype=np.int32)
    mode_x[1:M, 3:6] = capi.CONTINUOUS
    vt = np.array([60.0 * i / M for i in range(M + 1)])
    vX = np.zeros((M + 1, 12))
    for i in range(M + 1):
        vX[i, 0] = 20.0 * i / M
        if i < M:
            vX[i, 6:] = 0.001
    vX[:, 3:6] = 0.3                                       # moving, so that every component of the state takes part
    assert ctx.problem_set(mode_t, mode_x, vt, vX) == 26
    z = np.concatenate([vX[:M].ravel(), vt[1:]])
    return ctx, o, mode_t, perturbed(z, B, rel=0.05, seed=5), N


def build_covid(B=3, N=10, variant="exact"):
    """testCovid19's layout at M = 4: fixed tf = 30 days, S / E / I free at tf."""
    from socp_amd import capi
    from oracle.oracle import Oracle, MODEL_COVID
    o = Oracle(MODEL_COVID, step_nbr=N)
    ctx = capi.Context(capi.MODEL_COVID19)
    set_variant(ctx, variant)
    ctx.set_step_number(N)
    p = ctx.get_params()
    p[:3] = [3.4, 14.0, 5.0]
    ctx.set_params(p)
    o.set_params(p)
    M = 4
    Xi = np.array([0.93, 0.003, 0.01, 0.057, -0.001, 0.001, 0.0, 0.0])
    time = np.array([30.0 * i / M for i in range(M + 1)])
    X = np.zeros((M + 1, 8))
    X[0], X[M, 3] = Xi, 0.6
    nodes = np.stack([Xi] + [o.traj(0.0, Xi, time[i]) for i in range(1, M)])
    mode_t = [capi.FIXED] + [capi.CONTINUOUS] * (M - 1) + [capi.FIXED]
    mode_x = np.zeros((M + 1, 4), dtype=np.int32)
    mode_x[1:M] = capi.CONTINUOUS
    mode_x[M, :3] = capi.FREE
    assert ctx.problem_set(mode_t, mode_x, time, X) == 32
    return ctx, o, mode_t, perturbed(nodes.ravel(), B, rel=0.02, seed=3), N


LAYOUTS = {
    "goddard_B1_M1": lambda v="exact": build_goddard_fixed(1, 1, 10, v),
    "goddard_B23_M3": lambda v="exact": build_goddard_fixed(23, 3, 10, v),          # 69 lanes: a full workgroup and a partial one
    "goddard_c1_M6_free_tf": lambda v="exact": build_goddard_c1(5, 10, v),
    "goddard_n87_mu2_0_free_interior_times": lambda v="exact": build_goddard_n87(3, 10, v),
    "dint_wp_M2_free_interior_time": lambda v="exact": build_dint_wp(4, 10, v),
    "covid19_M4": lambda v="exact": build_covid(3, 10, v),
    "goddard_c1_M6_one_step": lambda v="exact": build_goddard_c1(2, 1, v),
}
_REF = {}


def oracle_reference(name):
    """The oracle-driven reference of a layout, computed once and shared (read-only) by the tests that need it."""
    if name not in _REF:
        ctx, o, mode_t, Z, N = LAYOUTS[name]()
        try:
            want = reference_oracle(o, ctx, mode_t, Z, N)
        finally:
            ctx.close()
        for a in want:
            a.setflags(write=False)
        _REF[name] = want
    return _REF[name]


# ---- 1. oracle parity, exact flavour, bit for bit --------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_oracle_parity_bit_for_bit(name):
    want = oracle_reference(name)
    ctx, o, mode_t, Z, N = LAYOUTS[name]()
    # (a segment that flies with the engine off costs exactly 0.0)
    assert np.all(np.isfinite(want[0])) and np.all(want[1] != 0.0), "the inputs of this test are meant to give a finite, nonzero cost"
    print("%s: cost %.6g .. %.6g" % (name, want[0].min(), want[0].max()))
    if "n87" in name:
        assert np.array_equal(lanes_of(ctx, mode_t, Z)[2], np.repeat(Z[:, [84, 85]], 6, axis=0)), "the switching times come from z"
    assert np.array_equal(u64(want[2]), u64(segment_ends(ctx, mode_t, Z))), "Xend is what integrate_batch gives for the segment"
    check_whole(run_host(ctx, Z), want, name + ", host form")
    check_whole(run_dev(ctx, Z), want, name + ", _dev form")
    ctx.close()


# ---- 2. composition parity on the GPU, exact flavour, bit for bit ------------------------------------------------------------

def build_vtol(variant="exact", N=8):
    from socp_amd import capi
    F = np.load(os.path.join(ROOT, "tests", "golden", "vtol_flow.npz"))
    ctx = capi.Context(capi.MODEL_VTOLUAV)
    set_variant(ctx, variant)
    ctx.set_map(read_obstacles(os.path.join(ROOT, "tests", "golden", "vtol", "obstacles_synthetic"))[:2])      # a two-obstacle map
    ctx.set_params(F["path_4_params"])
    ctx.set_step_number(N)
    mode_t = F["path_4_mode_t"].astype(np.int32)[:3]       # the first two segments of the four-waypoint stage
    mode_x = F["path_4_mode_X"].astype(np.int32).reshape(5, 6)[[0, 1, 4]]
    xnode = np.zeros((3, 12))
    xnode[:, :6] = F["path_4_xd"].reshape(5, 6)[:3]
    z4 = F["path_4_z0"]
    assert ctx.problem_set(mode_t, mode_x, F["path_4_time"][:3], xnode) == 26
    z = np.concatenate([z4[:24], z4[48:50]])
    return ctx, list(mode_t), perturbed(z, 3, rel=0.01, seed=13), N


def build_lqr1d(N=10):
    from socp_amd import capi
    capi.plugin_load(os.path.join(ROOT, "socp_amd", "_build", "plugins", "liblqr1d_plugin.so"))
    p = capi.Context(1001, nparams=1)
    p.set_step_number(N)
    M = 4
    mode_t = [capi.FIXED] + [capi.CONTINUOUS] * (M - 1) + [capi.FREE]
    mode_x = np.zeros((M + 1, 2), dtype=np.int32)
    mode_x[1:M] = capi.CONTINUOUS
    Xn = np.zeros((M + 1, 4))
    Xn[M, 0] = 1.0
    assert p.problem_set(mode_t, mode_x, np.linspace(0.0, 1.0, M + 1), Xn) == 4 * M + 1
    rng = np.random.default_rng(2)
    Zp = rng.uniform(-2.0, 2.0, size=(9, 4 * M + 1)) * np.logspace(-1, 2, 9)[:, None]
    Zp[:, -1] = np.linspace(0.5, 6.0, 9)
    return p, mode_t, Zp, N


def test_composition_parity_goddard_agrees_with_the_oracle_reference():
    name = "goddard_c1_M6_free_tf"
    ctx, o, mode_t, Z, N = LAYOUTS[name]()
    comp = reference_composition(ctx, mode_t, Z, N)
    for a, b in zip(comp, oracle_reference(name)):
        assert np.array_equal(u64(a), u64(b)), "the two references differ"
    check_whole(run_dev(ctx, Z), comp, "goddard, composition")
    ctx.close()


def test_composition_parity_vtol_with_a_two_obstacle_map():
    ctx, mode_t, Z, N = build_vtol()
    assert ctx.has_cost() and len(ctx.get_map()) == 2
    want = reference_composition(ctx, mode_t, Z, N)
    assert np.all(np.isfinite(want[0])) and np.all(want[0] != 0.0)
    assert np.array_equal(u64(want[2]), u64(segment_ends(ctx, mode_t, Z)))
    check_whole(run_host(ctx, Z), want, "vtolUAV, host form")
    check_whole(run_dev(ctx, Z), want, "vtolUAV, _dev form")
    ctx.close()


def test_composition_parity_plugin_model():
    p, mode_t, Z, N = build_lqr1d()
    assert p.has_cost()
    want = reference_composition(p, mode_t, Z, N)
    assert np.all(np.isfinite(want[0])) and np.all(want[0] > 0.0)           # int u^2 / 2
    assert np.array_equal(u64(want[2]), u64(segment_ends(p, mode_t, Z)))
    check_whole(run_host(p, Z), want, "lqr1d, host form")
    check_whole(run_dev(p, Z), want, "lqr1d, _dev form")
    p.close()


# ---- 3. per-problem blocks ---------------------------------------------------------------------------------------------

def test_per_problem_blocks_equal_single_row_contexts():
    """B = 7, every row with its own KD, node times and node states: _blocks, and socp_problem_set_blocks_dev + _dev with
    socp_problem_blocks_all_smooth 0 and 1, against seven single-row calls on a context set to the row's own data."""
    ctx, o, mode_t, Z, N = build_goddard_c1(B=7)
    prob, _ = goddard_c1_problem(o)
    B = 7
    base = np.concatenate([ctx.get_params(), [0.0, 0.0]])
    params = np.tile(base, (B, 1))
    params[:, 2] = [0.0, 50.0, 120.0, 310.0, 400.0, 10.0, 200.0]
    time = np.tile(prob.time, (B, 1))
    time[:, 0] = [0.0, 0.001, 0.002, -0.001, 0.003, 0.0005, -0.002]      # the FIXED initial time is the one the timeline reads
    xnode = np.tile(prob.xnode.ravel(), (B, 1)) * (1.0 + 0.01 * np.arange(B))[:, None]
    rows = []
    for b in range(B):
        ctx.set_params(params[b, :8])
        ctx.set_switching_times(params[b, 8:])
        ctx.problem_set(prob.mode_t, prob.mode_x, time[b], xnode[b].reshape(7, 14))
        r = ctx.cost_batch(Z[b:b + 1], xend=True)
        rows.append((r["cost"][0], r["total"][0], r["xend"][0]))
    want = tuple(np.stack([r[k] for r in rows]) for k in range(3))
    assert len(np.unique(want[1])) == B
    ctx.set_params(base[:8])
    ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode)
    r = ctx.cost_batch(Z, params=params, time=time, xnode=xnode, xend=True)
    for k, key in enumerate(("cost", "total", "xend")):
        assert np.array_equal(u64(r[key]), u64(want[k])), "_blocks: " + key
    # _blocks restores the context's own blocks: the shared-parameter call afterwards is the plain one
    plain = ctx.cost_batch(Z)
    assert not np.array_equal(plain["total"], want[1])
    for smooth in (0, 1):
        ctx._chk(ctx.L.socp_problem_blocks_all_smooth(ctx.h, smooth))
        check_whole(run_dev(ctx, Z, blocks=(params, time, xnode)), want, "set_blocks_dev + _dev, all_smooth = %d" % smooth)
    ctx._chk(ctx.L.socp_problem_blocks_all_smooth(ctx.h, 0))
    assert np.array_equal(u64(ctx.cost_batch(Z)["total"]), u64(plain["total"]))
    ctx.close()


# ---- 4. degenerate segments ------------------------------------------------------------------------------------------------

def test_zero_length_and_backward_segments_and_null_outputs():
    from socp_amd import capi
    ctx, o, _, _, N = build_goddard_c1()
    prob, _ = goddard_c1_problem(o)
    mode_t = [capi.FIXED] * 5
    mode_x = np.zeros((5, 7), dtype=np.int32)
    mode_x[1:4] = capi.CONTINUOUS
    t = np.array([0.0, 0.02, 0.02, 0.015, 0.04])          # segment 1 has zero length, segment 2 runs backward
    assert ctx.problem_set(mode_t, mode_x, t, prob.xnode[:5]) == 56
    Z = perturbed(prob.xnode[:4].ravel(), 3, seed=5)
    want = reference_oracle(o, ctx, mode_t, Z, N)
    assert np.all(u64(want[0][:, 1:3]) == 0), "+0.0"
    assert np.array_equal(want[2][:, 1:3], Z.reshape(3, 4, 14)[:, 1:3]) and np.all(want[0][:, [0, 3]] != 0.0)
    for run, form in ((run_host, "host form"), (run_dev, "_dev form")):
        got = run(ctx, Z)
        check_whole(got, want, "degenerate segments, " + form)
        assert np.all(got[0][:12].reshape(3, 4)[:, 1:3] == 0), "the bits of +0.0"
        check_whole(run(ctx, Z, total=False), (want[0], None, want[2]), "NULL total, " + form)
        check_whole(run(ctx, Z, xend=False), (want[0], want[1], None), "NULL Xend, " + form)
        check_whole(run(ctx, Z, total=False, xend=False), (want[0], None, None), "NULL total and Xend, " + form)
    ctx.close()


# ---- 5. throughput flavour -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_fast_flavour_within_the_composition_s_own_deviation(name):
    """e_new <= 2 e_old + 16 ulp of the largest magnitude, for cost and Xend (see the module docstring).
    The e_new / e_old pairs are printed by this test; profiles/cost_gpu_tests.txt keeps them (not measured yet)."""
    from socp_amd import capi
    ctx, o, mode_t, Z, N = LAYOUTS[name]("fast")
    B, M, s = len(Z), ctx.M, ctx.s
    ctx.set_variant(capi.VARIANT_LANE_EXACT)
    exact = run_dev(ctx, Z)
    ctx.set_variant(capi.VARIANT_LANE_FAST)
    comp = reference_composition(ctx, mode_t, Z, N)
    failures = []
    for run, form in ((run_host, "host"), (run_dev, "dev")):
        got = run(ctx, Z)
        for k, (group, size) in enumerate((("cost", B * M), ("total", B), ("xend", B * M * s))):
            assert np.all(got[k][size:] == SENT), "guard words behind %s were written" % group
            new, ref, old = got[k][:size].view(np.float64), exact[k][:size].view(np.float64), np.ravel(comp[k])
            assert np.all(np.isfinite(new)) and np.all(np.isfinite(ref))
            e_new, e_old = float(np.max(np.abs(new - ref))), float(np.max(np.abs(old - ref)))
            bar = 2.0 * e_old + 16.0 * EPS * float(np.max(np.abs(ref)))
            print("fast %s %s form, %s: e_new %.3e  e_old %.3e  bar %.3e" % (name, form, group, e_new, e_old, bar))
            if group != "total" and not e_new <= bar:
                failures.append((form, group, e_new, e_old, bar))
    ctx.close()
    assert not failures, failures


def test_fast_flavour_at_ten_thousand_steps_meets_the_project_bar():
    """Goddard single shooting, B = 64, M = 1, N = 10 000: |cost_fast - cost_exact| <= 1e-8 max(1, |cost|), the project's stated
    bar for the throughput flavour.  The figures the tests print belong in profiles/cost_gpu_tests.txt (not measured yet)."""
    from socp_amd import capi
    # the bench's inputs: the whole flight, costates within 1e-3 of the converged ones (sweep.goddard_starts)
    ctx, o, mode_t, Z, N = build_goddard_fixed(64, 1, 10000, "fast", tf=GODDARD_TF, eps=1e-3)
    fast = ctx.cost_batch(Z, xend=True)
    ctx.set_variant(capi.VARIANT_LANE_EXACT)
    exact = ctx.cost_batch(Z, xend=True)
    ctx.close()
    assert np.all(np.isfinite(exact["cost"])) and np.all(exact["cost"] > 0.0)
    dev = np.abs(fast["cost"] - exact["cost"]) / np.maximum(1.0, np.abs(exact["cost"]))
    devX = np.abs(fast["xend"] - exact["xend"]) / np.maximum(1.0, np.abs(exact["xend"]))
    print("fast vs exact at N = 10000, B = 64: cost %.6g .. %.6g, max deviation / max(1, |cost|) = %.3e; Xend %.3e"
          % (exact["cost"].min(), exact["cost"].max(), dev.max(), devX.max()))
    assert dev.max() <= 1e-8


# ---- 6. errors ---------------------------------------------------------------------------------------------------------

def test_errors_leave_the_context_unchanged_and_counters():
    from socp_amd import capi
    name = "goddard_B23_M3"
    want = oracle_reference(name)
    ctx, o, mode_t, Z, N = LAYOUTS[name]()
    B, M, s = len(Z), ctx.M, ctx.s
    Zc = np.ascontiguousarray(Z)
    cost, tot, xe = np.zeros(B * M), np.zeros(B), np.zeros(B * M * s)
    p = lambda a: a.ctypes.data_as(DP)  # noqa: E731
    L, h = ctx.L, ctx.h
    t0, l0 = ctx.counters()
    assert L.socp_cost_batch(h, -1, p(Zc), p(cost), p(tot), p(xe)) == capi.ERR_ARG
    assert L.socp_cost_batch_dev(h, -1, None, None, None, None) == capi.ERR_ARG
    assert L.socp_cost_batch(h, B, None, p(cost), p(tot), p(xe)) == capi.ERR_ARG
    assert L.socp_cost_batch(h, B, p(Zc), None, p(tot), p(xe)) == capi.ERR_ARG
    assert L.socp_cost_batch_dev(h, B, None, None, None, None) == capi.ERR_ARG
    assert L.socp_cost_batch_blocks(h, B, None, None, 0, None, None, p(cost), None, None) == capi.ERR_ARG
    params = np.tile(np.concatenate([ctx.get_params(), [0.0, 0.0]]), (B, 1))
    for stride in (8, 9, 11):
        assert L.socp_cost_batch_blocks(h, B, p(Zc), p(params), stride, None, None, p(cost), p(tot), p(xe)) == capi.ERR_ARG, stride
    assert "nparams + 2" in L.socp_last_error(h).decode()
    assert L.socp_cost_batch(h, 0, None, None, None, None) == capi.OK and L.socp_cost_batch_dev(h, 0, None, None, None, None) == capi.OK
    assert L.socp_cost_batch_blocks(h, 0, None, None, 0, None, None, None, None, None) == capi.OK
    ctx.set_integrator(capi.INT_DOPRI5, 1e-8)
    assert L.socp_cost_batch(h, B, p(Zc), p(cost), p(tot), p(xe)) == capi.ERR_UNSUPPORTED
    assert "DOPRI5" in L.socp_last_error(h).decode()
    assert L.socp_cost_batch_dev(h, B, p(Zc), p(cost), None, None) == capi.ERR_UNSUPPORTED        # refused before anything is enqueued
    assert L.socp_cost_batch_blocks(h, B, p(Zc), p(params), 10, None, None, p(cost), p(tot), p(xe)) == capi.ERR_UNSUPPORTED
    ctx.set_integrator(capi.INT_RK4)
    assert ctx.counters() == (t0, l0), "nothing was launched or counted"
    assert np.all(cost == 0.0) and np.all(tot == 0.0) and np.all(xe == 0.0)
    assert ctx.has_cost()

    fresh = capi.Context(capi.MODEL_GODDARD)
    assert fresh.L.socp_cost_batch(fresh.h, 1, p(Zc), p(cost), None, None) == capi.ERR_ARG
    assert "no problem set" in fresh.L.socp_last_error(fresh.h).decode()
    assert fresh.has_cost()
    fresh.close()

    from test_gpu_interceptor import multi_shooting_problem, scenario_state
    from oracle.oracle import Oracle, MODEL_INTERCEPTOR
    Xs, Xf = scenario_state(gamma=1.49)
    iprob, iz = multi_shooting_problem(Oracle(MODEL_INTERCEPTOR), 4, X0=Xs, Xf=Xf)
    for variant in (capi.VARIANT_LANE_EXACT, capi.VARIANT_LANE_FAST):
        for integ in (capi.INT_RK4, capi.INT_DOPRI5):
            ci = capi.Context(capi.MODEL_INTERCEPTOR)
            ci.set_variant(variant)
            ci.set_integrator(integ, 1e-8)
            assert ci.problem_set(iprob.mode_t, iprob.mode_x, iprob.time, iprob.xnode) == iprob.n
            assert not ci.has_cost()
            ic = np.zeros(4)
            c0 = ci.counters()
            assert ci.L.socp_cost_batch(ci.h, 1, p(np.ascontiguousarray(iz)), p(ic), None, None) == capi.ERR_UNSUPPORTED
            assert ci.counters() == c0 and np.all(ic == 0.0)
            with pytest.raises(capi.SocpError):
                ci.cost_batch(iz[None, :])
            ci.close()

    # a valid call afterwards reproduces test 1's bits, and the counters advance by B M trajectories, 1 launch (+ 1 with total)
    check_whole(run_host(ctx, Z), want, "after the refused calls")
    t1, l1 = ctx.counters()
    assert t1 - t0 == B * M and l1 - l0 == 2
    check_whole(run_host(ctx, Z, total=False), (want[0], None, want[2]), "without total")
    t2, l2 = ctx.counters()
    assert t2 - t1 == B * M and l2 - l1 == 1
    ctx.close()


# ---- 7. device pointers held by torch; the sweep tool ------------------------------------------------------------------------

def test_device_pointer_form_with_torch_tensors_equals_the_host_form():
    import torch
    name = "goddard_c1_M6_free_tf"
    ctx, o, mode_t, Z, N = LAYOUTS[name]()
    B, M, s = len(Z), ctx.M, ctx.s
    host = ctx.cost_batch(Z, xend=True)
    dZ = torch.from_numpy(np.ascontiguousarray(Z)).cuda()
    dC = torch.full((B, M), float("nan"), dtype=torch.float64, device="cuda")
    dT = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
    dX = torch.full((B, M, s), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.cost_batch_dev(B, dZ.data_ptr(), dC.data_ptr(), dT.data_ptr(), dX.data_ptr())
    ctx.synchronize()
    for key, t in (("cost", dC), ("total", dT), ("xend", dX)):
        assert np.array_equal(u64(t.cpu().numpy()), u64(host[key])), key
    assert np.array_equal(u64(host["cost"]), u64(oracle_reference(name)[0]))
    ctx.close()


def test_sweep_tool_writes_the_costs_of_its_converged_chains(tmp_path):
    from socp_amd import capi, sweep
    out = str(tmp_path / "cost")
    run = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--starts", "64", "--rk4-steps", "100", "--cost-out", out],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    entry = rec["cost_rank0"]
    assert sorted(entry) == sorted(["chains", "min", "median", "max", "best_index", "wall_s", "file"])
    npz = np.load(entry["file"])
    assert entry["file"] == out + ".rank0.npz" and entry["chains"] == rec["converged"] == len(npz["total"]) > 0
    assert npz["cost"].shape == (entry["chains"], 1) and npz["z"].shape == (entry["chains"], 14)
    assert entry["min"] == npz["total"].min() and entry["max"] == npz["total"].max() and entry["min"] <= entry["median"] <= entry["max"]
    assert entry["best_index"] == npz["index"][np.argmin(npz["total"])]
    ctx = capi.Context(capi.MODEL_GODDARD)
    ctx.set_params(sweep.GODDARD_PARAMS)
    ctx.set_step_number(100)
    ctx.set_variant(capi.VARIANT_LANE_FAST)
    sweep.goddard_single_shooting_problem(ctx)
    direct = ctx.cost_batch(npz["z"])
    assert np.array_equal(u64(direct["total"]), u64(npz["total"])) and np.array_equal(u64(direct["cost"]), u64(npz["cost"]))
    ctx.close()
    # --model interceptor with --cost-out is an argument error, before any device work
    bad = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--model", "interceptor", "--cost-out", out], cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--cost-out" in bad.stderr
