"""GPU: the batched Move(tf) and re-grid (socp_move_batch[_dev] / _blocks, socp_regrid_batch_dev / _blocks) against the COMPOSITION
of the existing entry points on the same context -- for every row b: ctx.timeline(z_b), capi.move_segment for the segment and the
target of every query, ctx.integrate_batch(tl[seg], target, z_b[s seg .. s seg + s), sw = what the residual uses for the row), with
set_params / problem_set per row where a row has its own blocks -- and against tests/move_reference.py on the CPU oracle.
Comparisons are on uint64 views (NaN-safe) of WHOLE outputs: the host forms' arrays are pre-filled with NaN, the _dev forms' torch
tensors carry a 64-double sentinel band on each side, which must come back untouched.  Reference-order flavour: bit equality
throughout.  Throughput flavour: see test_throughput_flavour."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import move_reference
from test_gpu_trace_batch import SENT, GUARD, u64, model_sw, vtol_ctx
from test_move_batch_cpu import stage3_shooting, stage4_structure, stage4_times

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "goddard_flow.json")))
Z3 = np.array(GOLD["goddard_N10_M6"][2]["z"])                    # stage 3 of testGoddard: M = 6, n = 85, KD = 310, mu2 = 0.2
Z4 = np.array(GOLD["goddard_N10_M6"][3]["z"])                    # stage 4: n = 87, FREE nodes 2, 4 and 6
G3_PARAMS = [3.5, 7.0, 310.0, 500.0, 1.0, 1.0, 0.2, -1.0]
G4_PARAMS = [3.5, 7.0, 310.0, 500.0, 1.0, 1.0, 0.0, -1.0]        # mu2 = 0, singularControl = -1
X0_STATE = [0.999949994, 1e-4, 0.01, 1e-10, 1e-10, 1e-10, 1.0]
EPS = 2.0 ** -52
DP = C.POINTER(C.c_double)
IP = C.POINTER(C.c_int)


# ---- cases: a context with its problem, the rows, the queries, and (optionally) per-row blocks -------------------------------

class Case:
    def __init__(self, name, ctx, mode_t, mode_x, time, xnode, Z, TQ, blocks=None, custom_traj=False):
        self.name, self.ctx, self.mode_t, self.mode_x = name, ctx, list(mode_t), np.asarray(mode_x)
        self.time, self.xnode = np.asarray(time, dtype=np.float64), np.asarray(xnode, dtype=np.float64)
        self.Z, self.TQ = np.ascontiguousarray(Z, dtype=np.float64), np.ascontiguousarray(TQ, dtype=np.float64)
        self.blocks, self.custom_traj = blocks, custom_traj
        self.base = ctx.get_params()
        self.base_sw = np.empty(2)
        assert ctx.L.socp_ctx_get_switching_times(ctx.h, self.base_sw.ctypes.data_as(DP)) == 0

    def set_variant(self, fast):
        from socp_amd import capi
        self.ctx.set_variant(capi.VARIANT_LANE_FAST if fast else capi.VARIANT_LANE_EXACT)

    def row_problem(self, b):
        """The context holds row b's own problem: what a per-row block means."""
        if self.blocks is None:
            return
        P, T, XN = self.blocks
        npar = len(self.base)
        if P is not None:
            self.ctx.set_params(P[b, :npar])
            self.ctx.set_switching_times(P[b, npar:])
        self.ctx.problem_set(self.mode_t, self.mode_x, self.time if T is None else T[b], self.xnode if XN is None else XN[b].reshape(self.xnode.shape))

    def restore(self):
        if self.blocks is None:
            return
        self.ctx.set_params(self.base)
        self.ctx.set_switching_times(self.base_sw)
        self.ctx.problem_set(self.mode_t, self.mode_x, self.time, self.xnode)

    def kw(self):
        if self.blocks is None:
            return {}
        return dict(params=self.blocks[0], time=self.blocks[1], xnode=self.blocks[2])


def compose(case):
    """(Xq[B][K][s], tout[B][K], seg[B][K]) from the existing entry points."""
    from socp_amd import capi
    ctx, s = case.ctx, case.ctx.s
    B, K = case.TQ.shape
    Xq, tout, segs = np.empty((B, K, s)), np.empty((B, K)), np.empty((B, K), dtype=int)
    for b in range(B):
        case.row_problem(b)
        z = case.Z[b]
        tl = ctx.timeline(z)
        sw = model_sw(ctx, case.mode_t, tl, case.custom_traj)
        pick = [capi.move_segment(tl, q) for q in case.TQ[b]]
        segs[b] = [p[0] for p in pick]
        tout[b] = [p[1] for p in pick]
        X0 = np.stack([z[s * g:s * g + s] for g in segs[b]])
        Xq[b] = ctx.integrate_batch(tl[segs[b]], tout[b], X0, sw=None if case.custom_traj else np.tile(sw, (K, 1)))
    case.restore()
    return Xq, tout, segs


def dev_buffer(torch, count):
    t = torch.from_numpy(np.full(count + 2 * GUARD, SENT, dtype=np.uint64).view(np.float64)).cuda()
    return t, t.data_ptr() + 8 * GUARD


def dev_payload(t, count, what):
    a = t.cpu().numpy().view(np.uint64)
    assert np.all(a[:GUARD] == SENT), what + ": the band in front of the buffer was written"
    assert np.all(a[GUARD + count:] == SENT), what + ": the band behind the buffer was written"
    return a[GUARD:GUARD + count]


class dev_blocks:
    """socp_problem_set_blocks_dev with the case's blocks for the duration of a _dev call."""

    def __init__(self, case):
        self.case = case

    def __enter__(self):
        import torch
        case = self.case
        if case.blocks is None:
            return self
        self.keep = [None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda() for a in case.blocks]
        ptr = [None if t is None else t.data_ptr() for t in self.keep]
        case.ctx._chk(case.ctx.L.socp_problem_set_blocks_dev(case.ctx.h, ptr[0], case.blocks[0].shape[1] if case.blocks[0] is not None else 0,
                                                             ptr[1], ptr[2]))
        torch.cuda.synchronize()
        return self

    def __exit__(self, *exc):
        if self.case.blocks is not None:
            self.case.ctx.L.socp_problem_set_blocks_dev(self.case.ctx.h, None, 0, None, None)


def run_dev(case, want_tout=True):
    import torch
    ctx, s = case.ctx, case.ctx.s
    B, K = case.TQ.shape
    dZ, dQ = torch.from_numpy(case.Z).cuda(), torch.from_numpy(case.TQ).cuda()
    tX, pX = dev_buffer(torch, B * K * s)
    tT, pT = dev_buffer(torch, B * K)
    with dev_blocks(case):
        ctx.move_batch_dev(B, dZ.data_ptr(), K, dQ.data_ptr(), pX, pT if want_tout else None)
        ctx.synchronize()
        torch.cuda.synchronize()
    Xq = dev_payload(tX, B * K * s, case.name + " Xq").reshape(B, K, s)
    T = dev_payload(tT, B * K, case.name + " tout")
    if not want_tout:
        assert np.all(T == SENT), "tout was written although NULL was passed"
    return Xq, T.reshape(B, K)


def check_exact(case):
    """Host form and _dev form against the composition, whole buffers, bit for bit."""
    wantX, wantT, segs = compose(case)
    assert case.custom_traj or np.all(np.isfinite(wantX)), case.name + ": the inputs of this test are meant to stay finite"
    Xq, T = case.ctx.move_batch(case.Z, case.TQ, tout=True, **case.kw())
    bad = np.argwhere(u64(Xq) != u64(wantX))
    assert len(bad) == 0, (case.name, "host form, first differing (b, k, c):", bad[:5].tolist(), segs.tolist())
    assert np.array_equal(u64(T), u64(wantT)), (case.name, "host form tout")
    Xonly = case.ctx.move_batch(case.Z, case.TQ, **case.kw())
    assert np.array_equal(u64(Xonly), u64(wantX)), (case.name, "host form without tout")
    dX, dT = run_dev(case)
    assert np.array_equal(dX, u64(wantX)) and np.array_equal(dT, u64(wantT)), (case.name, "_dev form")
    dX, _ = run_dev(case, want_tout=False)
    assert np.array_equal(dX, u64(wantX)), (case.name, "_dev form without tout")
    return wantX, wantT, segs


# ---- Goddard -----------------------------------------------------------------------------------------------------------------------

def goddard_layout():
    from socp_amd import capi
    M, d = 6, 7
    mode_t = [capi.FIXED] + [capi.CONTINUOUS] * (M - 1) + [capi.FREE]
    mode_x = np.zeros((M + 1, d), dtype=np.int32)
    mode_x[1:M] = capi.CONTINUOUS
    mode_x[M, 3:7] = capi.FREE
    time = np.array([0.0 + i * (0.1 - 0.0) / M for i in range(M + 1)])          # what the flow's shooting object holds: its first grid
    X = np.zeros((M + 1, 14))
    X[0, :7] = X0_STATE
    X[M, 0] = 1.01
    return mode_t, mode_x, time, X


def goddard_ctx(params, step_nbr=10):
    from socp_amd import capi
    ctx = capi.Context(capi.MODEL_GODDARD)
    ctx.set_variant(capi.VARIANT_LANE_EXACT)
    ctx.set_params(params)
    ctx.set_step_number(step_nbr)
    return ctx


def queries_everywhere(tl):
    """23 queries of a row: both ends, every interior node time exactly, segment midpoints and quarter points, and the out-of-range ones."""
    tl = np.asarray(tl)
    M = len(tl) - 1
    mids = [0.5 * (tl[i] + tl[i + 1]) for i in range(M)]
    quarters = [tl[i] + 0.25 * (tl[i + 1] - tl[i]) for i in range(M)]
    q = [tl[0], tl[M]] + list(tl[1:M]) + mids + quarters + [-1.0, 1.0, float("nan"), np.nextafter(tl[M], np.inf)]
    return np.array(q)


def case1():
    """M = 6, n = 85; B = 3, K = 23 (69 lanes: a full wave and a partial one); rows 1 and 2 with their own KD, node times, altitude target."""
    ctx = goddard_ctx(G3_PARAMS)
    mode_t, mode_x, time, X = goddard_layout()
    assert ctx.problem_set(mode_t, mode_x, time, X) == 85
    B = 3
    Z = np.tile(Z3, (B, 1))
    P = np.tile(np.array(G3_PARAMS + [0.0227, 0.08]), (B, 1))
    P[:, 2] = [310.0, 200.0, 400.0]
    T = np.tile(time, (B, 1))
    T[1, 0], T[2, 0] = 0.001, -0.002                       # the FIXED initial time is the one the timeline reads
    T[1:, 1:] *= 1.1
    XN = np.tile(X.ravel(), (B, 1))
    XN[:, 6 * 14] = [1.01, 1.012, 1.008]
    TQ = np.empty((B, 23))
    for b in range(B):
        ctx.problem_set(mode_t, mode_x, T[b], X)
        TQ[b] = queries_everywhere(ctx.timeline(Z[b]))
    ctx.problem_set(mode_t, mode_x, time, X)
    return Case("goddard M6", ctx, mode_t, mode_x, time, X, Z, TQ, blocks=(P, T, XN))


def stage4_problem():
    from oracle.oracle import FREE
    mode_xf = np.zeros(7, dtype=np.int32)
    mode_xf[3:7] = FREE
    mode_t, mode_x = stage4_structure(mode_xf)
    time = stage4_times(Z3[-1])
    X = np.zeros((7, 14))
    X[0, :7] = X0_STATE
    X[6, 0] = 1.01
    return mode_t, mode_x, time, X


def case2(disordered=False):
    """n = 87: the stage-4 structure, FREE nodes 2 and 4 (the model's switching times) and 6; K = 9 over all six segments."""
    ctx = goddard_ctx(G4_PARAMS)
    mode_t, mode_x, time, X = stage4_problem()
    assert ctx.problem_set(mode_t, mode_x, time, X) == 87
    Z = np.tile(Z4, (2, 1))
    Z[1, :84] *= 1.0 + 1e-4                                # a second row, so that a read outside row b shows
    if disordered:
        Z[0, 85] = Z4[86] * 1.2                            # FREE node 4 above tf: nodes 3 .. 6 are out of order
        Z[1, 85] = Z4[86] * 1.05
    TQ = np.empty((2, 9))
    for b in range(2):
        tl = ctx.timeline(Z[b])
        lo, hi = min(tl), max(tl)
        TQ[b] = [0.5 * (tl[i] + tl[i + 1]) for i in range(6)] + [tl[2], tl[4], tl[6]]
        if disordered:
            TQ[b, 6:] = [0.5 * (tl[6] + hi), lo + 0.9 * (tl[6] - lo), tl[5]]
    return Case("goddard n87" + (" disordered" if disordered else ""), ctx, mode_t, mode_x, time, X, Z, TQ)


@pytest.fixture(scope="module")
def c1():
    case = case1()
    yield case
    case.ctx.close()


def test_goddard_m6_rows_with_their_own_blocks(c1, built):
    wantX, wantT, segs = check_exact(c1)
    assert set(segs[0].tolist()) == {0, 1, 2, 3, 4, 5}
    # the selection of row 0: t0, te, the interior node times (each integrates the WHOLE previous segment), ..., -1, +1, NaN, te+
    assert segs[0, :7].tolist() == [0, 5, 0, 1, 2, 3, 4] and segs[0, -4:].tolist() == [5, 5, 5, 5]
    assert np.all(wantT[0, -4:] == Z3[-1]) and np.array_equal(u64(wantX[0, 0]), u64(Z3[:14]))
    assert not np.array_equal(wantX[0], wantX[1]) and not np.array_equal(wantX[1], wantX[2])
    # row 0 on the CPU oracle: OracleShooting.move
    o, sh, z, _ = stage3_shooting()
    for k, q in enumerate(c1.TQ[0]):
        assert np.array_equal(u64(sh.move(q)), u64(wantX[0, k])), (k, q)
    # a B = 1 call of row 0, shared-parameter kernel: the same bits
    X1, T1 = c1.ctx.move_batch(c1.Z[:1], c1.TQ[:1], tout=True)
    assert np.array_equal(u64(X1[0]), u64(wantX[0])) and np.array_equal(u64(T1[0]), u64(wantT[0]))


def test_blocks_form_restores_the_contexts_own_blocks(c1):
    """_blocks puts the caller's blocks in force for the call only: blocks set with socp_problem_set_blocks_dev before are back after."""
    import torch
    ctx = c1.ctx
    wantX, _, _ = compose(c1)
    own = torch.from_numpy(np.ascontiguousarray(np.tile(c1.blocks[0][1], (3, 1)))).cuda()        # KD = 200 for every row
    ctx._chk(ctx.L.socp_problem_set_blocks_dev(ctx.h, own.data_ptr(), 10, None, None))
    try:
        ctx.move_batch(c1.Z, c1.TQ, **c1.kw())
        dZ, dQ = torch.from_numpy(c1.Z).cuda(), torch.from_numpy(c1.TQ).cuda()
        tX, pX = dev_buffer(torch, 3 * 23 * 14)
        ctx.move_batch_dev(3, dZ.data_ptr(), 23, dQ.data_ptr(), pX, None)
        ctx.synchronize()
    finally:
        ctx.L.socp_problem_set_blocks_dev(ctx.h, None, 0, None, None)
    got = dev_payload(tX, 3 * 23 * 14, "own blocks").reshape(3, 23, 14)
    ctx.set_param("KD", 200.0)
    ctx.set_switching_times(c1.blocks[0][1, 8:])
    want = ctx.move_batch(c1.Z, c1.TQ)                       # the shared-parameter kernel at KD = 200
    ctx.set_params(c1.base)
    ctx.set_switching_times(c1.base_sw)
    assert np.array_equal(got, u64(want)) and not np.array_equal(got, u64(wantX))


def test_goddard_stage4_structure_switching_times_from_z(built):
    from oracle.oracle import Oracle, Problem, MODEL_GODDARD
    case = case2()
    wantX, wantT, segs = check_exact(case)
    assert segs[0].tolist() == [0, 1, 2, 3, 4, 5, 1, 3, 5]
    o = Oracle(MODEL_GODDARD, step_nbr=10)
    o.set_params(G4_PARAMS)
    prob = Problem(7, case.mode_t, case.mode_x, case.time, case.xnode)
    for b in range(2):
        tl = o.timeline(prob, case.Z[b])
        assert np.array_equal(tl, case.ctx.timeline(case.Z[b]))
        o.set_switching([tl[2], tl[4]])
        for k, q in enumerate(case.TQ[b]):
            X, target = move_reference.move(o, tl, case.Z[b], 14, q)
            assert target == wantT[b, k] and np.array_equal(u64(X), u64(wantX[b, k])), (b, k)
    case.ctx.close()


def test_disordered_timeline_stays_inside_the_row():
    case = case2(disordered=True)
    tl = case.ctx.timeline(case.Z[0])
    assert tl[4] > tl[6] and tl[5] > tl[6] and tl[3] > tl[2]
    wantX, wantT, segs = check_exact(case)
    assert segs.max() <= 5 and len(set(segs[0].tolist())) >= 3
    case.ctx.close()


def test_free_initial_time_double_integrator():
    """M = 2, mode_t[0] FREE: tl(0) is the unknown z[s M]; B = 2, K = 5 with a query below it."""
    from socp_amd import capi
    ctx = capi.Context(capi.MODEL_DOUBLE_INTEGRATOR)
    ctx.set_variant(capi.VARIANT_LANE_EXACT)
    ctx.set_step_number(10)
    mode_t = [capi.FREE, capi.CONTINUOUS, capi.FIXED]
    mode_x = np.zeros((3, 6), dtype=np.int32)
    mode_x[1] = capi.CONTINUOUS
    time = np.array([0.0, 5.0, 10.0])
    X = np.zeros((3, 12))
    X[2, 0], X[2, 1] = 10.0, 15.0
    assert ctx.problem_set(mode_t, mode_x, time, X) == 25
    rng = np.random.default_rng(4)
    Z = np.empty((2, 25))
    Z[:, :24] = rng.uniform(-1.0, 1.0, (2, 24)) * np.tile([1, 1, 1, 0.5, 0.5, 0.5, 0.01, 0.01, 0.01, 0.01, 0.01, 0.01], 2)
    Z[:, 24] = [1.0, 2.5]
    TQ = np.array([[1.0, 0.5, 3.0, 5.5, 10.0], [2.5, 0.0, 6.25, 8.0, 11.0]])
    case = Case("double integrator, FREE t0", ctx, mode_t, mode_x, time, X, Z, TQ)
    assert np.array_equal(ctx.timeline(Z[1]), [2.5, 6.25, 10.0])
    wantX, wantT, segs = check_exact(case)
    assert wantT[0].tolist() == [1.0, 10.0, 3.0, 5.5, 10.0] and segs[0].tolist() == [0, 1, 0, 0, 1]
    assert segs[1].tolist() == [0, 1, 0, 1, 1] and np.array_equal(u64(wantX[1, 0]), u64(Z[1, :12]))
    ctx.close()


def test_adaptive_integrator_goddard():
    from socp_amd import capi
    ctx = goddard_ctx(G3_PARAMS)
    ctx.set_integrator(capi.INT_DOPRI5, 1e-8)
    mode_t, mode_x, time, X = goddard_layout()
    assert ctx.problem_set(mode_t, mode_x, time, X) == 85
    Z = np.tile(Z3, (2, 1))
    Z[1, 7:14] *= 1.0 + 1e-3
    Z[1, -1] *= 1.1
    TQ = np.stack([queries_everywhere(ctx.timeline(z))[[0, 3, 8, 13, 1]] for z in Z])
    case = Case("goddard dopri5", ctx, mode_t, mode_x, time, X, Z, TQ)
    wantX, _, segs = check_exact(case)
    ctx.set_integrator(capi.INT_RK4)
    fixed = ctx.move_batch(Z, TQ)
    assert not np.array_equal(fixed, wantX)                # the move follows the context's integrator
    ctx.close()


# ---- other models: B = 3, K = 4 ----------------------------------------------------------------------------------------------------------

def spread_queries(ctx, Z, K=4):
    """node time, inside the first segment, inside the last, beyond the end"""
    out = []
    for z in Z:
        tl = ctx.timeline(z)
        M = len(tl) - 1
        out.append([tl[min(1, M)], tl[0] + 0.3 * (tl[1] - tl[0]), tl[M - 1] + 0.6 * (tl[M] - tl[M - 1]), tl[M] + 1.0][:K])
    return np.array(out)


def covid_case():
    from socp_amd import capi
    ctx = capi.Context(capi.MODEL_COVID19)
    ctx.set_variant(capi.VARIANT_LANE_EXACT)
    ctx.set_params([3.4, 14, 5, 1, 0.1, 1, -10, 20])
    ctx.set_step_number(10)
    M = 3
    mode_t = [capi.FIXED] + [capi.CONTINUOUS] * (M - 1) + [capi.FIXED]
    mode_x = np.zeros((M + 1, 4), dtype=np.int32)
    mode_x[1:M] = capi.CONTINUOUS
    mode_x[M, :3] = capi.FREE
    Xi = np.array([0.93, 0.003, 0.01, 0.057, -0.001, 0.001, 0.0, 0.0])
    time = np.array([0.0, 10.0, 20.0, 30.0])
    X = np.zeros((M + 1, 8))
    X[0] = Xi
    X[1:M] = ctx.integrate_batch(np.zeros(M - 1), time[1:M], np.repeat(Xi[None, :], M - 1, axis=0))
    X[M, 3] = 0.6
    assert ctx.problem_set(mode_t, mode_x, time, X) == 24
    rng = np.random.default_rng(9)
    Z = X[:M].ravel()[None, :] * (1.0 + 0.01 * rng.uniform(-1, 1, (3, 24)))
    return Case("covid19", ctx, mode_t, mode_x, time, X, Z, spread_queries(ctx, Z))


def vtol_case():
    ctx, mode_t, Z = vtol_ctx("exact")
    F = np.load(os.path.join(ROOT, "tests", "golden", "vtol_flow.npz"))
    mode_x = F["path_4_mode_X"].astype(np.int32).reshape(5, 6)[[0, 1, 2, 4]]
    xnode = np.zeros((4, 12))
    xnode[:, :6] = F["path_4_xd"].reshape(5, 6)[:4]
    return Case("vtolUAV", ctx, mode_t, mode_x, F["path_4_time"][:4], xnode, Z, spread_queries(ctx, Z))


def interceptor_case(adaptive):
    """Fixed step: the analytical guess, whose first segment starts with a chart change.  Adaptive: nodes along the CONVERGED scenario-1
    trajectory (tests/golden) -- the adaptive integrator takes thousands of steps on the guess."""
    from socp_amd import capi
    from oracle.oracle import Oracle, MODEL_INTERCEPTOR
    from test_gpu_interceptor import multi_shooting_problem, scenario_state
    o = Oracle(MODEL_INTERCEPTOR)
    if adaptive:
        gold = json.load(open(os.path.join(ROOT, "tests", "golden", "interceptor_flow.json")))["scenario1_xtol1e-12"][-1]["z"]
        Xf = np.zeros(12)
        Xf[:6] = [12000, 1000, 0.0, np.pi / 8, 5475000 / 6378145.0, 42000 / 6378145.0]
        prob, z = multi_shooting_problem(o, 4, tf=gold[12], X0=np.array(gold[:12]), Xf=Xf)
    else:
        Xs, Xf = scenario_state(gamma=1.49)               # starts with a chart change
        prob, z = multi_shooting_problem(o, 4, X0=Xs, Xf=Xf)
    ctx = capi.Context(capi.MODEL_INTERCEPTOR)
    ctx.set_variant(capi.VARIANT_LANE_EXACT)
    ctx.set_step_number(6)
    if adaptive:
        ctx.set_integrator(capi.INT_DOPRI5, 1e-8)
    assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == prob.n
    Z = np.tile(z, (3, 1))
    Z[1, 6:12] *= 1.0 + 1e-3
    Z[2, 6:12] *= 1.0 - 1e-3
    return Case("interceptor " + ("dopri5" if adaptive else "rk4"), ctx, prob.mode_t, prob.mode_x, prob.time, prob.xnode, Z, spread_queries(ctx, Z),
                custom_traj=True)


def plugin_case():
    from socp_amd import capi
    capi.plugin_load(os.path.join(ROOT, "socp_amd", "_build", "plugins", "liblqr1d_plugin.so"))
    p = capi.Context(1001, nparams=1)
    p.set_step_number(10)
    M = 4
    mode_t = [capi.FIXED] + [capi.CONTINUOUS] * (M - 1) + [capi.FREE]
    mode_x = np.zeros((M + 1, 2), dtype=np.int32)
    mode_x[1:M] = capi.CONTINUOUS
    Xn = np.zeros((M + 1, 4))
    Xn[M, 0] = 1.0
    time = np.linspace(0.0, 1.0, M + 1)
    assert p.problem_set(mode_t, mode_x, time, Xn) == 4 * M + 1
    rng = np.random.default_rng(2)
    Z = rng.uniform(-2.0, 2.0, size=(3, 4 * M + 1))
    Z[:, -1] = [0.5, 2.0, 6.0]
    return Case("lqr1d plugin", p, mode_t, mode_x, time, Xn, Z, spread_queries(p, Z))


OTHER_MODELS = {"covid19": covid_case, "vtolUAV": vtol_case, "interceptor-rk4": lambda: interceptor_case(False),
                "interceptor-dopri5": lambda: interceptor_case(True), "lqr1d": plugin_case}


@pytest.mark.parametrize("model", sorted(OTHER_MODELS))
def test_other_models(model):
    case = OTHER_MODELS[model]()
    assert case.TQ.shape == (3, 4)
    wantX, wantT, segs = check_exact(case)
    assert segs[0, 0] == 0 and segs[0, 2] == len(case.mode_t) - 2 and wantT[0, 3] == case.ctx.timeline(case.Z[0])[-1]
    case.ctx.close()


# ---- throughput flavour ------------------------------------------------------------------------------------------------------------

def rel_dev(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def existing_paths_deviation(case):
    """d0: the throughput flavour's integrate_batch against the last kept row of its trace_batch(stride >= step_nbr), over the
    segments of every row -- two existing instantiations of the same arithmetic."""
    ctx, s = case.ctx, case.ctx.s
    M = len(case.mode_t) - 1
    rows, count = ctx.trace_batch(case.Z, stride=1 << 20, **case.kw())
    d0 = 0.0
    for b, z in enumerate(case.Z):
        case.row_problem(b)
        tl = ctx.timeline(z)
        sw = model_sw(ctx, case.mode_t, tl, case.custom_traj)
        Xf = ctx.integrate_batch(tl[:M], tl[1:], z[:s * M].reshape(M, s), sw=None if case.custom_traj else np.tile(sw, (M, 1)))
        last = np.stack([rows[b, i, count[b, i] - 1, 1:1 + s] for i in range(M)])
        assert np.all(np.isfinite(Xf)) and np.all(np.isfinite(last))
        d0 = max(d0, rel_dev(last, Xf))
    case.restore()
    return d0


FAST_CASES = dict(OTHER_MODELS, **{"goddard-M6": case1, "goddard-n87": case2})


@pytest.mark.parametrize("name", sorted(FAST_CASES))
def test_throughput_flavour(name):
    """The move of the throughput flavour is a third instantiation of arithmetic two existing paths of that flavour already
    contract each in its own way.  d0 = their deviation from each other on the same segments, relative to max(1, |x|); the move may
    differ from the composition (integrate_batch) by at most 4 max(d0, 2^-52) -- the factor 4 for a third instantiation's own
    contraction choices -- and must stay within the flavour's project bar 1e-8 max(1, |x|) of the reference-order result.
    The figures this test prints belong in profiles/move_gpu_tests.txt."""
    case = FAST_CASES[name]()
    ref, refT, _ = compose(case)
    case.set_variant(True)
    d0 = existing_paths_deviation(case)
    wantX, wantT, _ = compose(case)
    Xq, T = case.ctx.move_batch(case.Z, case.TQ, tout=True, **case.kw())
    dX, dT = run_dev(case)
    assert np.array_equal(u64(T), u64(wantT)) and np.array_equal(dT, u64(wantT)) and np.array_equal(u64(wantT), u64(refT))
    assert np.array_equal(dX, u64(Xq)), "host and _dev form of one flavour"
    dev, to_ref = rel_dev(Xq, wantX), rel_dev(Xq, ref)
    bar = 4.0 * max(d0, EPS)
    print("move fast %-20s d0 %.3e  |move - composition| %.3e  bar %.3e  |move - reference order| %.3e" % (name, d0, dev, bar, to_ref))
    case.ctx.close()
    assert dev <= bar, (name, dev, bar)
    assert to_ref <= 1e-8, (name, to_ref)


# ---- re-grid -----------------------------------------------------------------------------------------------------------------------

def regrid_inputs():
    ctx = goddard_ctx(G3_PARAMS)
    mode_t, mode_x, time, X = goddard_layout()
    assert ctx.problem_set(mode_t, mode_x, time, X) == 85
    mode_t2, _, _, _ = stage4_problem()
    tf = Z3[-1]
    B = 3
    Z = np.tile(Z3, (B, 1))
    T2 = np.tile(stage4_times(tf), (B, 1))
    T2[1, 4] = tf * 1.1                                    # a FREE node beyond tf: the time is packed as given, the state is Move's clamp
    P = np.tile(np.array(G3_PARAMS + [0.0227, 0.08]), (B, 1))
    P[2, 2] = 200.0
    return ctx, mode_t2, Z, T2, P


def regrid_on_the_oracle(Z, T2, P, mode_t2):
    from oracle.oracle import Oracle, Problem, MODEL_GODDARD
    mode_t, mode_x, time, X = goddard_layout()
    out = []
    for b in range(len(Z)):
        o = Oracle(MODEL_GODDARD, step_nbr=10)
        o.set_params(P[b, :8])
        tl = o.timeline(Problem(7, mode_t, mode_x, time, X), Z[b])
        out.append(move_reference.regrid(o, tl, Z[b], 14, mode_t2, T2[b]))
    return out


def test_regrid_against_the_oracle_host_and_dev_forms(built):
    import torch
    from socp_amd import capi
    ctx, mode_t2, Z, T2, P = regrid_inputs()
    B = len(Z)
    want = regrid_on_the_oracle(Z, T2, P, mode_t2)
    assert ctx.regrid_num_param(mode_t2) == 87
    r = ctx.regrid_batch(Z, mode_t2, T2, params=P)
    assert r["z"].shape == (B, 87) and r["xnode"].shape == (B, 7, 14) and r["time"] is not T2 and np.array_equal(r["time"], T2)
    for b in range(B):
        assert np.array_equal(u64(r["z"][b]), u64(want[b]["z"])), b
        assert np.array_equal(u64(r["xnode"][b]), u64(want[b]["xnode"])), b
        assert np.array_equal(r["z"][b, 84:], T2[b, [2, 4, 6]]), b
    assert r["z"][1, 85] == T2[1, 4] > Z3[-1] and np.array_equal(u64(r["xnode"][1, 4]), u64(r["xnode"][1, 6]))
    assert not np.array_equal(r["z"][0], r["z"][2]), "the per-row KD is honoured"
    # xnode2 = NULL
    r0 = ctx.regrid_batch(Z, mode_t2, T2, params=P, want_xnode=False)
    assert r0["xnode"] is None and np.array_equal(u64(r0["z"]), u64(r["z"]))
    # _dev form, with and without xnode2
    case = Case("regrid", ctx, *goddard_layout(), Z, T2, blocks=(P, None, None))
    dZ, dT = torch.from_numpy(np.ascontiguousarray(Z)).cuda(), torch.from_numpy(np.ascontiguousarray(T2)).cuda()
    for with_x in (True, False):
        tZ2, pZ2 = dev_buffer(torch, B * 87)
        tX2, pX2 = dev_buffer(torch, B * 7 * 14)
        t0, l0 = ctx.counters()
        with dev_blocks(case):
            ctx.regrid_batch_dev(B, dZ.data_ptr(), mode_t2, dT.data_ptr(), pZ2, pX2 if with_x else None)
            ctx.synchronize()
            torch.cuda.synchronize()
        t1, l1 = ctx.counters()
        assert (t1 - t0, l1 - l0) == (B * 7, 2)
        assert np.array_equal(dev_payload(tZ2, B * 87, "Z2").reshape(B, 87), u64(r["z"]))
        X2 = dev_payload(tX2, B * 7 * 14, "xnode2")
        assert np.array_equal(X2.reshape(B, 7, 14), u64(r["xnode"])) if with_x else np.all(X2 == SENT)
    # all-FIXED target, M2 = 1 and a CONTINUOUS interior: n2 = s M2, no time entries
    r1 = ctx.regrid_batch(Z[:1], [capi.FIXED, capi.CONTINUOUS, capi.FIXED], [[0.0, 0.1, 0.2]])
    assert r1["z"].shape == (1, 28) and np.array_equal(u64(r1["z"][0, :14]), u64(Z3[:14]))
    ctx.close()


def test_refusals_leave_the_context_unchanged():
    from socp_amd import capi
    ctx, mode_t2, Z, T2, P = regrid_inputs()
    L, h = ctx.L, ctx.h
    B, K = 3, 7
    Zc, Tc, Pc = np.ascontiguousarray(Z), np.ascontiguousarray(T2), np.ascontiguousarray(P)
    Xq, Z2 = np.zeros((B, K, 14)), np.zeros((B, 87))
    mt = np.array(mode_t2, dtype=np.int32)
    bad_mode = mt.copy()
    bad_mode[3] = 3
    d, ip = (lambda a: a.ctypes.data_as(DP)), (lambda a: a.ctypes.data_as(IP))
    import torch
    before = ctx.move_batch(Z, T2, params=P)
    # blocks set with socp_problem_set_blocks_dev are in force while the calls are refused: KD = 200 for every row
    own = torch.from_numpy(np.ascontiguousarray(np.tile(P[2], (B, 1)))).cuda()
    dZ, dQ = torch.from_numpy(Zc).cuda(), torch.from_numpy(Tc).cuda()

    def with_own_blocks():
        tX, pX = dev_buffer(torch, B * K * 14)
        ctx.move_batch_dev(B, dZ.data_ptr(), K, dQ.data_ptr(), pX, None)
        ctx.synchronize()
        return dev_payload(tX, B * K * 14, "own blocks").copy()
    ctx._chk(L.socp_problem_set_blocks_dev(h, own.data_ptr(), 10, None, None))
    torch.cuda.synchronize()
    own_before = with_own_blocks()
    assert not np.array_equal(own_before.reshape(B, K, 14)[0], u64(before[0])), "the blocks in force are read"
    params0, count0 = ctx.get_params(), ctx.counters()
    refused = [
        L.socp_move_batch(h, -1, d(Zc), K, d(Tc), d(Xq), None),
        L.socp_move_batch(h, B, d(Zc), -1, d(Tc), d(Xq), None),
        L.socp_move_batch(h, B, None, K, d(Tc), d(Xq), None),
        L.socp_move_batch(h, B, d(Zc), K, None, d(Xq), None),
        L.socp_move_batch(h, B, d(Zc), K, d(Tc), None, None),
        L.socp_move_batch_dev(h, B, None, K, None, None, None),
        L.socp_move_batch_dev(h, -1, None, K, None, None, None),
        L.socp_move_batch_blocks(h, B, d(Zc), d(Pc), 9, None, None, K, d(Tc), d(Xq), None),
        L.socp_regrid_batch_blocks(h, B, d(Zc), d(Pc), 11, None, None, 6, ip(mt), d(Tc), d(Z2), None),
        L.socp_regrid_batch_blocks(h, B, d(Zc), None, 0, None, None, 6, ip(bad_mode), d(Tc), d(Z2), None),
        L.socp_regrid_batch_blocks(h, B, d(Zc), None, 0, None, None, 0, ip(mt), d(Tc), d(Z2), None),
        L.socp_regrid_batch_blocks(h, B, d(Zc), None, 0, None, None, 256, ip(mt), d(Tc), d(Z2), None),
        L.socp_regrid_batch_blocks(h, -1, d(Zc), None, 0, None, None, 6, ip(mt), d(Tc), d(Z2), None),
        L.socp_regrid_batch_blocks(h, B, d(Zc), None, 0, None, None, 6, None, d(Tc), d(Z2), None),
        L.socp_regrid_batch_blocks(h, B, d(Zc), None, 0, None, None, 6, ip(mt), None, d(Z2), None),
        L.socp_regrid_batch_dev(h, B, None, 6, ip(mt), None, None, None),
        L.socp_regrid_batch_dev(h, B, None, 6, ip(bad_mode), None, None, None),
        L.socp_regrid_num_param(h, 6, ip(bad_mode)),
        L.socp_regrid_num_param(h, 0, ip(mt)),
        L.socp_regrid_num_param(h, 256, ip(mt)),
    ]
    assert refused == [capi.ERR_ARG] * len(refused), refused
    assert np.array_equal(ctx.get_params(), params0) and ctx.counters() == count0
    assert np.all(Xq == 0.0) and np.all(Z2 == 0.0)
    assert np.array_equal(with_own_blocks(), own_before), "the blocks in force before the refusals are in force after them"
    L.socp_problem_set_blocks_dev(h, None, 0, None, None)
    assert np.array_equal(u64(ctx.move_batch(Z, T2, params=P)), u64(before))          # parameters, problem and blocks as they were
    fresh = capi.Context(capi.MODEL_GODDARD)
    assert fresh.L.socp_move_batch(fresh.h, B, d(Zc), K, d(Tc), d(Xq), None) == capi.ERR_ARG
    assert "no problem set" in fresh.L.socp_last_error(fresh.h).decode()
    assert fresh.L.socp_regrid_batch_blocks(fresh.h, B, d(Zc), None, 0, None, None, 6, ip(mt), d(Tc), d(Z2), None) == capi.ERR_ARG
    assert fresh.counters() == (0, 0)
    fresh.close()
    ctx.close()


def test_counters_and_empty_shapes(c1):
    from socp_amd import capi
    ctx = c1.ctx
    L, h = ctx.L, ctx.h
    mode_t2, _, _, _ = stage4_problem()
    mt = np.array(mode_t2, dtype=np.int32)
    t0, l0 = ctx.counters()
    assert L.socp_move_batch(h, 0, None, 5, None, None, None) == capi.OK and L.socp_move_batch(h, 3, None, 0, None, None, None) == capi.OK
    assert L.socp_move_batch_dev(h, 0, None, 5, None, None, None) == capi.OK and L.socp_move_batch_dev(h, 3, None, 0, None, None, None) == capi.OK
    assert L.socp_move_batch_blocks(h, 0, None, None, 0, None, None, 5, None, None, None) == capi.OK
    assert L.socp_regrid_batch_dev(h, 0, None, 6, mt.ctypes.data_as(IP), None, None, None) == capi.OK
    assert L.socp_regrid_batch_blocks(h, 0, None, None, 0, None, None, 6, mt.ctypes.data_as(IP), None, None, None) == capi.OK
    assert ctx.counters() == (t0, l0)                       # nothing was launched
    X = ctx.move_batch(c1.Z, np.empty((3, 0)))
    assert X.shape == (3, 0, 14) and ctx.counters() == (t0, l0)
    X, T = ctx.move_batch(np.empty((0, 85)), np.empty((0, 5)), tout=True)
    assert X.shape == (0, 5, 14) and T.shape == (0, 5) and ctx.counters() == (t0, l0)
    ctx.move_batch(c1.Z, c1.TQ)
    t1, l1 = ctx.counters()
    assert (t1 - t0, l1 - l0) == (3 * 23, 1)
    ctx.regrid_batch(c1.Z, mode_t2, stage4_times(Z3[-1]))
    t2, l2 = ctx.counters()
    assert (t2 - t1, l2 - l1) == (3 * 7, 2)


# ---- the flow's stage 4 in batch ---------------------------------------------------------------------------------------------------

def test_stage4_of_the_flow_from_a_batched_regrid():
    """testGoddard.cpp:115-156 for B = 4 solutions at once: re-grid the stage-3 solution onto the singular-arc structure, then
    solve stage 4 as PLAIN chains with every chain's own node times and node states.  Row 0 is the program's own stage 4."""
    from socp_amd import capi
    ctx3 = goddard_ctx(G3_PARAMS)
    mode_t, mode_x, time, X = goddard_layout()
    assert ctx3.problem_set(mode_t, mode_x, time, X) == 85
    mode_t2, mode_x2, time2, X2 = stage4_problem()
    B = 4
    T2 = np.tile(stage4_times(Z3[-1]), (B, 1))
    for b, f in zip((1, 2, 3), (0.98, 1.02, 1.05)):
        s1, s2, tf = 0.0227 * f, 0.08 * f, Z3[-1]
        T2[b] = [0.0, s1 / 2, s1, (s2 + s1) / 2, s2, (s2 + tf) / 2, tf]
    r = ctx3.regrid_batch(np.tile(Z3, (B, 1)), mode_t2, T2)
    ctx3.close()
    ctx4 = goddard_ctx(G4_PARAMS)
    assert ctx4.problem_set(mode_t2, mode_x2, time2, X2) == 87 == r["z"].shape[1]
    res = ctx4.chains_solve(r["z"], kind=capi.CHAIN_PLAIN, params=np.tile(G4_PARAMS, (B, 1)), time_goal=r["time"],
                            x_goal=r["xnode"].reshape(B, -1), xtol=1e-6)
    print("stage 4 in batch: info %s nfev %s" % (res["info"].tolist(), res["nfev"].tolist()))
    assert res["info"][0] == 1 and res["nfev"][0] == 101
    assert np.array_equal(res["z"][0], Z4)
    assert res["z"].shape == (B, 87) and len(res["info"]) == B
    ctx4.close()


# ---- the sweep tool ----------------------------------------------------------------------------------------------------------------

def test_sweep_tool_regrid_out(tmp_path):
    from socp_amd import capi, sweep
    out = str(tmp_path / "regrid")
    run = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--starts", "8", "--segments", "2", "--rk4-steps", "10", "--variant", "exact",
                          "--regrid-segments", "4", "--regrid-out", out], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("{")][-1])
    F = np.load(out + ".rank0.npz")
    k = int(rec["converged"])
    assert rec["regrid_rank0"]["count"] == k == len(F["index"]) and rec["regrid_rank0"]["n2"] == 14 * 4 + 1 and rec["regrid_rank0"]["seconds"] > 0
    assert k >= 1, "the sweep of this test is meant to converge for some starts"
    ctx = capi.Context(capi.MODEL_GODDARD)
    ctx.set_params(sweep.GODDARD_PARAMS)
    ctx.set_step_number(10)
    ctx.set_variant(capi.VARIANT_LANE_EXACT)
    sweep.goddard_multiple_shooting_problem(ctx, 2)
    # that run's solve, repeated: the rows the tool moved are its converged rows
    Z0 = sweep.goddard_multiple_shooting_starts(ctx, sweep.goddard_starts(8, 0.05), 2)
    res = ctx.chains_solve(Z0, kind=capi.CHAIN_PLAIN, xtol=1e-8)
    conv = np.where(res["info"] == 1)[0]
    assert np.array_equal(F["index"], conv) and np.array_equal(F["source"], res["z"][conv])
    mode_t2 = [capi.FIXED] + [capi.CONTINUOUS] * 3 + [capi.FREE]
    T2 = np.stack([np.linspace(tl[0], tl[-1], 5) for tl in (ctx.timeline(z) for z in F["source"])])
    r = ctx.regrid_batch(F["source"], mode_t2, T2)
    assert np.array_equal(u64(F["z"]), u64(r["z"])) and np.array_equal(u64(F["xnode"]), u64(r["xnode"])) and np.array_equal(F["time"], T2)
    assert np.array_equal(F["z"][:, -1], F["source"][:, -1])            # the free final time travels as given
    ctx.close()
