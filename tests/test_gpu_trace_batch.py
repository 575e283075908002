"""GPU: the batched trace (socp_trace_batch[_dev], capi.Context.trace_batch) against the COMPOSITION of the single-trajectory
entry points on the same context -- for every (b, i): timeline(z_b), integrate_dense_aux(t1, t2, X_start, sw), eval_batch for
u and H at every row with the row's aux pair, capi.trace_kept_rows for the kept indices.  Comparisons are on uint64 views
(NaN-safe) of the WHOLE output buffer, pre-filled with a sentinel bit pattern and followed by guard words, so a write outside
[b][i][0 .. min(count, cap)) fails.  Exact flavour: bit equality.  Throughput flavour (kernels contracted differently from
each other): count and kept indices equal, and per column group e_new = max|batch_fast - composition_exact| within
2 e_old + 16 ulp of the group's largest magnitude, e_old = max|composition_fast - composition_exact| -- the existing path's own
deviation; the factor 2 because both are independent contractions of the same arithmetic.
Measured on an MI355X (profiles/trace_gpu_tests.txt): e_new = e_old in every group -- Goddard X 8.6e-8, u 9.7e-15, H 8.0e-8;
vtolUAV X 7.1e-15, u 4.1e-15, H 4.2e-17."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import goddard_c1_problem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = np.uint64(0x7FF8DEADBEEF0001)            # a NaN no kernel produces
SENT_I = np.int32(-559038737)
GUARD = 64
EPS = 2.0 ** -52


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def sentinel_rows(size):
    return np.full(size + GUARD, SENT, dtype=np.uint64).view(np.float64)


def model_sw(ctx, mode_t, tl, custom_traj):
    """The aux pair a segment starts with: the times of the first two FREE nodes below M (socp_problem_set), else the context's."""
    from socp_amd import capi
    sw = np.empty(2)
    assert ctx.L.socp_ctx_get_switching_times(ctx.h, sw.ctypes.data_as(C.POINTER(C.c_double))) == 0
    if not custom_traj:
        free = [j for j in range(len(mode_t) - 1) if mode_t[j] == capi.FREE]
        for k, j in enumerate(free[:2]):
            sw[k] = tl[j]
    return sw


def compose_full(ctx, Z, mode_t, custom_traj=False, per_row=None):
    """full[b][i] = every row the existing entry points give for segment i of z_b: array [R][W]."""
    from socp_amd import capi
    s, M, W = ctx.s, len(mode_t) - 1, ctx.trace_width()
    full = []
    for b, z in enumerate(Z):
        if per_row is not None:
            per_row(b)
        tl = ctx.timeline(z)
        sw = model_sw(ctx, mode_t, tl, custom_traj)
        segs, T, X, A = [], [], [], []
        for i in range(M):
            t, x, aux = ctx.integrate_dense_aux(tl[i], tl[i + 1], z[s * i:s * (i + 1)], sw=None if custom_traj else sw, cap=4096)
            assert len(t) < 4096, "the composition's own buffer was too small for this segment"
            segs.append(len(t))
            T.append(t), X.append(x), A.append(aux)
        T, X, A = np.concatenate(T), np.concatenate(X), np.concatenate(A)
        u = ctx.eval_batch(capi.EVAL_CONTROL, T, X, sw=A)
        H = ctx.eval_batch(capi.EVAL_HAMILTONIAN, T, X, sw=A)
        rows = np.concatenate([T[:, None], X, u, H, A], axis=1)
        assert rows.shape[1] == W
        full.append(np.split(rows, np.cumsum(segs)[:-1]))
    return full


def expected(full, stride, cap, W):
    from socp_amd import capi
    B, M = len(full), len(full[0])
    rows = np.full((B, M, cap, W), SENT, dtype=np.uint64)
    count = np.zeros((B, M), dtype=np.int32)
    for b in range(B):
        for i in range(M):
            kept = capi.trace_kept_rows(len(full[b][i]), stride)
            count[b, i] = len(kept)
            k = min(len(kept), cap)
            rows[b, i, :k] = u64(full[b][i][kept[:k]])
    return rows, count


def run_host(ctx, Z, stride, cap):
    """socp_trace_batch on guarded, sentinel-filled buffers: (whole rows buffer as uint64, whole count buffer)."""
    B, M, W = len(Z), ctx.M, ctx.trace_width()
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    rows = sentinel_rows(B * M * cap * W)
    count = np.full(B * M + GUARD, SENT_I, dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    ctx._chk(ctx.L.socp_trace_batch(ctx.h, B, Z.ctypes.data_as(dp), stride, cap, rows.ctypes.data_as(dp), count.ctypes.data_as(ip)))
    return rows.view(np.uint64), count


def run_dev(ctx, Z, stride, cap, blocks=None):
    import torch
    B, M, W = len(Z), ctx.M, ctx.trace_width()
    dZ = torch.from_numpy(np.ascontiguousarray(Z, dtype=np.float64)).cuda()
    dR = torch.from_numpy(sentinel_rows(B * M * cap * W)).cuda()
    dC = torch.from_numpy(np.full(B * M + GUARD, SENT_I, dtype=np.int32)).cuda()
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
        ctx.trace_batch_dev(B, dZ.data_ptr(), stride, cap, dR.data_ptr(), dC.data_ptr())
        ctx.synchronize()
        torch.cuda.synchronize()
    finally:
        if blocks is not None:
            ctx.L.socp_problem_set_blocks_dev(ctx.h, None, 0, None, None)
    return dR.cpu().numpy().view(np.uint64), dC.cpu().numpy()


def check_whole(got_rows, got_count, want_rows, want_count, what=""):
    n, m = want_rows.size, want_count.size
    assert np.array_equal(got_count[:m].reshape(want_count.shape), want_count), (what, got_count[:m], want_count)
    assert np.all(got_count[m:] == SENT_I), what + ": guard words behind count were written"
    assert np.all(got_rows[n:] == SENT), what + ": guard words behind rows were written"
    bad = np.argwhere(got_rows[:n].reshape(want_rows.shape) != want_rows)
    assert len(bad) == 0, (what, "first differing (b, i, row, column):", bad[:5].tolist())


# ---- Goddard, the testGoddard layout (M = 6, free tf, n = 85), step_nbr = 10, B = 11: 66 lanes = a second wave with two live lanes

def goddard_ctx(variant="exact", mu2=1.0, step_nbr=10):
    from socp_amd import capi
    from oracle.oracle import Oracle, MODEL_GODDARD
    o = Oracle(MODEL_GODDARD, step_nbr=step_nbr)
    o.set_param("mu2", mu2)
    prob, z = goddard_c1_problem(o)
    ctx = capi.Context(capi.MODEL_GODDARD)
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    ctx.set_param("mu2", mu2)
    ctx.set_step_number(step_nbr)
    assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == prob.n == 85
    return ctx, prob, z


def perturbed(z, B, rel=0.02, seed=7):
    rng = np.random.default_rng(seed)
    return z[None, :] * (1.0 + rel * rng.uniform(-1, 1, size=(B, len(z))))


@pytest.fixture(scope="module")
def goddard_case():
    ctx, prob, z = goddard_ctx()
    Z = perturbed(z, 11)
    full = compose_full(ctx, Z, prob.mode_t)
    yield ctx, prob, Z, full
    ctx.close()


@pytest.mark.parametrize("stride,want_count", [(1, 11), (4, 4), (10, 2), (25, 2)])
def test_goddard_strides_bit_equal_host_and_dev(goddard_case, stride, want_count):
    ctx, prob, Z, full = goddard_case
    W = ctx.trace_width()
    assert W == 1 + 14 + 3 + 1 + 2
    want_rows, want_cnt = expected(full, stride, 12, W)
    assert np.all(want_cnt == want_count)
    check_whole(*run_host(ctx, Z, stride, 12), want_rows, want_cnt, "host form")
    check_whole(*run_dev(ctx, Z, stride, 12), want_rows, want_cnt, "_dev form")


def test_goddard_cap_below_count_and_two_call_protocol(goddard_case):
    ctx, prob, Z, full = goddard_case
    W = ctx.trace_width()
    want_rows, want_cnt = expected(full, 1, 3, W)
    assert np.all(want_cnt == 11)                      # counted, not stored
    check_whole(*run_host(ctx, Z, 1, 3), want_rows, want_cnt, "cap = 3")
    check_whole(*run_dev(ctx, Z, 1, 3), want_rows, want_cnt, "cap = 3, _dev")
    rows, count = ctx.trace_batch(Z)                   # cap=None: the wrapper sizes the buffer itself and returns every row
    assert np.all(count == 11) and rows.shape[:3] == (11, 6, rows.shape[2]) and rows.shape[2] >= 11
    for b in range(11):
        for i in range(6):
            assert np.array_equal(u64(rows[b, i, :11]), u64(full[b][i]))
            assert np.all(np.isnan(rows[b, i, 11:]))


def test_goddard_bang_singular_off_switch_inside_a_segment():
    """mu2 = 0: the control law reads the switching times.  (a) the context's switching times, placed INSIDE segments of the fixed
    layout; (b) a layout with FREE interior times, whose switching times come from z."""
    from socp_amd import capi
    ctx, prob, z = goddard_ctx(mu2=0.0)
    W = ctx.trace_width()
    Z = perturbed(z, 3, rel=0.01)
    tl = ctx.timeline(Z[0])
    ctx.set_switching_times([0.5 * (tl[1] + tl[2]), 0.5 * (tl[3] + tl[4])])
    full = compose_full(ctx, Z, prob.mode_t)
    laws = set()
    for seg in full[0]:
        laws.update(np.round(np.linalg.norm(seg[:, 15:18], axis=1), 12).tolist())
        assert np.all(seg[:, W - 2] == 0.5 * (tl[1] + tl[2])) and np.all(seg[:, W - 1] == 0.5 * (tl[3] + tl[4]))
    assert 0.0 in laws and len(laws) >= 2, laws           # off after the second switch, bang before the first
    for stride in (1, 4):
        want = expected(full, stride, 12, W)
        check_whole(*run_host(ctx, Z, stride, 12), *want, "context switching times")
        check_whole(*run_dev(ctx, Z, stride, 12), *want, "context switching times, _dev")
    # (b) M = 3, both interior times FREE: sw0 = z[42], sw1 = z[43]
    mode_t = [capi.FIXED, capi.FREE, capi.FREE, capi.FREE]
    mode_x = np.zeros((4, 7), dtype=np.int32)
    mode_x[1:3] = capi.CONTINUOUS
    mode_x[3, 3:7] = capi.FREE
    assert ctx.problem_set(mode_t, mode_x, prob.time[[0, 2, 4, 6]], prob.xnode[[0, 2, 4, 6]]) == 45
    ctx.set_param("singularControl", -1.0)             # the singular arc computes its own control
    z3 = np.concatenate([prob.xnode[[0, 2, 4]].ravel(), prob.time[[2, 4, 6]]])
    Z3 = perturbed(z3, 4, rel=0.01, seed=11)
    full = compose_full(ctx, Z3, mode_t)
    for b in range(4):
        for i in range(3):
            assert np.all(full[b][i][:, W - 2] == Z3[b, 42]) and np.all(full[b][i][:, W - 1] == Z3[b, 43])
    assert np.all(np.linalg.norm(full[0][2][1:, 15:18], axis=1) == 0.0)      # past the second switching time: engine off
    for stride in (1, 3):
        want = expected(full, stride, 12, W)
        check_whole(*run_host(ctx, Z3, stride, 12), *want, "switching times from z")
        check_whole(*run_dev(ctx, Z3, stride, 12), *want, "switching times from z, _dev")
    ctx.close()


def test_goddard_per_problem_blocks():
    """B = 5, every row with its own KD, node times and node states; the checker sets parameters and the problem per row."""
    ctx, prob, z = goddard_ctx()
    W, B = ctx.trace_width(), 5
    Z = perturbed(z, B, seed=3)
    base = np.concatenate([ctx.get_params(), [0.0, 0.0]])
    params = np.tile(base, (B, 1))
    params[:, 2] = [0.0, 50.0, 120.0, 310.0, 400.0]
    time = np.tile(prob.time, (B, 1))
    time[:, 0] = [0.0, 0.001, 0.002, -0.001, 0.003]    # the FIXED initial time is the one the timeline reads
    xnode = np.tile(prob.xnode.ravel(), (B, 1)) * (1.0 + 0.01 * np.arange(B))[:, None]

    def per_row(b):
        ctx.set_params(params[b, :8])
        ctx.set_switching_times(params[b, 8:])
        ctx.problem_set(prob.mode_t, prob.mode_x, time[b], xnode[b].reshape(7, 14))
    full = compose_full(ctx, Z, prob.mode_t, per_row=per_row)
    assert not np.array_equal(full[0][0][-1], full[1][0][-1])
    ctx.set_params(base[:8])
    ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode)
    for stride in (1, 4):
        want_rows, want_cnt = expected(full, stride, 12, W)
        check_whole(*run_dev(ctx, Z, stride, 12, blocks=(params, time, xnode)), want_rows, want_cnt, "blocks, _dev")
        rows, count = ctx.trace_batch(Z, stride=stride, cap=12, params=params, time=time, xnode=xnode, fill=np.array([SENT]).view(np.float64)[0])
        assert np.array_equal(count, want_cnt) and np.array_equal(u64(rows), want_rows)
    ctx.close()


def test_zero_length_and_backward_segments():
    from socp_amd import capi
    ctx, prob, z = goddard_ctx()
    W = ctx.trace_width()
    mode_t = [capi.FIXED] * 5
    mode_x = np.zeros((5, 7), dtype=np.int32)
    mode_x[1:4] = capi.CONTINUOUS
    t = np.array([0.0, 0.02, 0.02, 0.015, 0.04])          # segment 1 has zero length, segment 2 runs backward
    assert ctx.problem_set(mode_t, mode_x, t, prob.xnode[:5]) == 56
    Z = perturbed(prob.xnode[:4].ravel(), 3, seed=5)
    full = compose_full(ctx, Z, mode_t)
    want_rows, want_cnt = expected(full, 4, 12, W)
    assert np.all(want_cnt[:, 1:3] == 1) and np.all(want_cnt[:, [0, 3]] == 4)
    check_whole(*run_host(ctx, Z, 4, 12), want_rows, want_cnt, "degenerate segments")
    check_whole(*run_dev(ctx, Z, 4, 12), want_rows, want_cnt, "degenerate segments, _dev")
    ctx.close()


def test_adaptive_integrator_goddard_and_plugin_model():
    """SOCP_INT_DOPRI5, tol 1e-8, stride 3: the number of rows is the integrator's own, lanes of one wave end with different counts."""
    from socp_amd import capi
    ctx, prob, z = goddard_ctx()
    ctx.set_integrator(capi.INT_DOPRI5, 1e-8)
    W = ctx.trace_width()
    Z = perturbed(z, 11, rel=0.002)
    Z[:, -1] = z[-1] * np.linspace(0.5, 2.0, 11)           # free tf: segments from short to long
    full = compose_full(ctx, Z, prob.mode_t)
    want_rows, want_cnt = expected(full, 3, 24, W)
    print("adaptive goddard: rows per segment %d .. %d, kept %d .. %d" % (min(len(s) for f in full for s in f), max(len(s) for f in full for s in f),
                                                                         want_cnt.min(), want_cnt.max()))
    assert len(np.unique(want_cnt.ravel()[:64])) > 1
    check_whole(*run_host(ctx, Z, 3, 24), want_rows, want_cnt, "adaptive")
    check_whole(*run_dev(ctx, Z, 3, 24), want_rows, want_cnt, "adaptive, _dev")
    # the two-call protocol's repeat: single shooting over the whole flight at a tolerance that needs more rows than the wrapper's
    # first guess of 64
    from socp_amd import sweep
    ctx.set_params(sweep.GODDARD_PARAMS)
    ctx.set_integrator(capi.INT_DOPRI5, 1e-13)
    sweep.goddard_single_shooting_problem(ctx)
    Z1 = sweep.goddard_starts(2, 1e-3)
    full = compose_full(ctx, Z1, [capi.FIXED, capi.FIXED])
    longest = max(len(s) for f in full for s in f)
    print("adaptive goddard single shooting, tol 1e-13: %s rows" % [len(f[0]) for f in full])
    assert longest > 64
    rows, count = ctx.trace_batch(Z1)
    assert rows.shape[2] == longest == count.max()
    for b in range(2):
        assert count[b, 0] == len(full[b][0]) and np.array_equal(u64(rows[b, 0, :count[b, 0]]), u64(full[b][0]))
    ctx.close()

    capi.plugin_load(os.path.join(ROOT, "socp_amd", "_build", "plugins", "liblqr1d_plugin.so"))
    p = capi.Context(1001, nparams=1)
    p.set_integrator(capi.INT_DOPRI5, 1e-8)
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
    Wp = p.trace_width()
    assert Wp == 1 + 4 + 1 + 1 + 2
    full = compose_full(p, Zp, mode_t)
    want_rows, want_cnt = expected(full, 3, 16, Wp)
    print("adaptive lqr1d: kept %d .. %d" % (want_cnt.min(), want_cnt.max()))
    check_whole(*run_host(p, Zp, 3, 16), want_rows, want_cnt, "plugin adaptive")
    check_whole(*run_dev(p, Zp, 3, 16), want_rows, want_cnt, "plugin adaptive, _dev")
    p.set_integrator(capi.INT_RK4)
    full = compose_full(p, Zp, mode_t)
    want = expected(full, 3, 16, Wp)
    check_whole(*run_dev(p, Zp, 3, 16), *want, "plugin fixed step, _dev")
    p.close()


@pytest.mark.parametrize("adaptive", [False, True])
def test_interceptor_stage_and_chart_columns_and_the_extra_final_row(adaptive):
    from socp_amd import capi
    from oracle.oracle import Oracle, MODEL_INTERCEPTOR
    import json
    from test_gpu_interceptor import multi_shooting_problem, scenario_state
    o = Oracle(MODEL_INTERCEPTOR)
    if adaptive:
        # nodes along the CONVERGED scenario-1 trajectory (tests/golden): the analytical guess below runs into states where the adaptive
        # integrator takes thousands of steps
        gold = json.load(open(os.path.join(ROOT, "tests", "golden", "interceptor_flow.json")))["scenario1_xtol1e-12"][-1]["z"]
        Xf = np.zeros(12)
        Xf[:6] = [12000, 1000, 0.0, np.pi / 8, 5475000 / 6378145.0, 42000 / 6378145.0]
        prob, z = multi_shooting_problem(o, 4, tf=gold[12], X0=np.array(gold[:12]), Xf=Xf)
    else:
        Xs, Xf = scenario_state(gamma=1.49)               # |cos(gamma)| < chartLimit: starts with a chart change
        prob, z = multi_shooting_problem(o, 4, X0=Xs, Xf=Xf)
    ctx = capi.Context(capi.MODEL_INTERCEPTOR)
    ctx.set_step_number(6)
    if adaptive:
        ctx.set_integrator(capi.INT_DOPRI5, 1e-8)
    assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == prob.n
    W = ctx.trace_width()
    assert W == 1 + 12 + 2 + 1 + 2
    Z = np.tile(z, (2, 1))
    Z[1, 6:12] *= 1.0 + 1e-3
    full = compose_full(ctx, Z, prob.mode_t, custom_traj=True)
    aux = np.concatenate([s[:, W - 2:] for s in full[0]])
    print("interceptor %s: rows per segment %s, stages %s, charts %s" % ("adaptive" if adaptive else "fixed step", [len(s) for s in full[0]],
                                                                        sorted(set(aux[:, 0])), sorted(set(aux[:, 1]))))
    if not adaptive:
        assert set(aux[:, 0]) == {0.0, 1.0} and 2.0 in set(aux[:, 1]), "both stages and a chart change are in the traced rows"
        assert [len(s) for s in full[0]] == [8, 8, 8, 15]   # stage start + 6 steps + the extra row; the last segment crosses t1 = 20 s
    cap = max(len(s) for f in full for s in f)
    for stride in (1, 4):
        want_rows, want_cnt = expected(full, stride, cap, W)
        got = run_host(ctx, Z, stride, cap)
        check_whole(*got, want_rows, want_cnt, "interceptor")
        check_whole(*run_dev(ctx, Z, stride, cap), want_rows, want_cnt, "interceptor, _dev")
        # the extra final row (the state ComputeTraj returns, the flags it leaves) is always the last kept one
        rows = got[0][:want_rows.size].reshape(want_rows.shape)
        for i in range(4):
            assert np.array_equal(rows[0, i, want_cnt[0, i] - 1], u64(full[0][i][-1]))
    ctx.close()


# ---- vtolUAV with the synthetic obstacle file, M = 3, B = 3, step_nbr = 8

def read_obstacles(path):
    rows = [ln.split() for ln in open(path).read().splitlines()]
    n = int(rows[1][0])
    return np.array([[float(rows[3 + i][0])] + [float(v) for v in rows[4 + n + i][:3]] + [float(v) for v in rows[5 + 2 * n + i][:3]]
                     for i in range(n)])


def vtol_ctx(variant):
    from socp_amd import capi
    F = np.load(os.path.join(ROOT, "tests", "golden", "vtol_flow.npz"))
    ctx = capi.Context(capi.MODEL_VTOLUAV)
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    ctx.set_map(read_obstacles(os.path.join(ROOT, "tests", "golden", "vtol", "obstacles_synthetic")))
    ctx.set_params(F["path_4_params"])
    ctx.set_step_number(8)
    mode_t = F["path_4_mode_t"].astype(np.int32)[:4]       # the first three segments of the four-waypoint stage
    mode_x = F["path_4_mode_X"].astype(np.int32).reshape(5, 6)[[0, 1, 2, 4]]
    xnode = np.zeros((4, 12))
    xnode[:, :6] = F["path_4_xd"].reshape(5, 6)[:4]
    z4 = F["path_4_z0"]
    assert ctx.problem_set(mode_t, mode_x, F["path_4_time"][:4], xnode) == 39
    z = np.concatenate([z4[:36], z4[48:51]])
    return ctx, mode_t, perturbed(z, 3, rel=0.01, seed=13)


def test_vtol_with_the_synthetic_obstacle_map():
    ctx, mode_t, Z = vtol_ctx("exact")
    W = ctx.trace_width()
    full = compose_full(ctx, Z, mode_t)
    assert all(len(s) == 9 for f in full for s in f)
    for stride in (1, 3):
        want = expected(full, stride, 10, W)
        check_whole(*run_host(ctx, Z, stride, 10), *want, "vtolUAV")
        check_whole(*run_dev(ctx, Z, stride, 10), *want, "vtolUAV, _dev")
    ctx.close()


# ---- throughput flavour: the existing path's own deviation is the yardstick

def fast_flavour_check(name, make_ctx, S, NU):
    from socp_amd import capi
    ctx, mode_t, Z = make_ctx()
    W = ctx.trace_width()
    ctx.set_variant(capi.VARIANT_LANE_EXACT)
    exact = compose_full(ctx, Z, mode_t)
    ctx.set_variant(capi.VARIANT_LANE_FAST)
    fast = compose_full(ctx, Z, mode_t)
    failures = []
    for stride in (1, 4):
        cap = 12
        ex_rows, ex_cnt = expected(exact, stride, cap, W)
        fa_rows, fa_cnt = expected(fast, stride, cap, W)
        assert np.array_equal(ex_cnt, fa_cnt)
        for form, (rows, count) in (("host", run_host(ctx, Z, stride, cap)), ("dev", run_dev(ctx, Z, stride, cap))):
            m = ex_cnt.size
            assert np.array_equal(count[:m].reshape(ex_cnt.shape), ex_cnt) and np.all(count[m:] == SENT_I)
            rows, guard = rows[:ex_rows.size].reshape(ex_rows.shape), rows[ex_rows.size:]
            assert np.all(guard == SENT)
            assert np.array_equal(rows == SENT, ex_rows == SENT), "rows outside [0, min(count, cap)) were written, or kept rows are missing"
            live = ex_rows[..., 0] != SENT
            new, old, ref = rows.view(np.float64)[live], fa_rows.view(np.float64)[live], ex_rows.view(np.float64)[live]
            assert np.array_equal(u64(new[:, 0]), u64(old[:, 0])), "times of the kept rows"          # t carries no model arithmetic
            assert np.array_equal(u64(new[:, W - 2:]), u64(old[:, W - 2:])), "aux columns"
            fin = np.isfinite(ref)
            assert np.array_equal(np.isfinite(new), fin) and np.array_equal(np.isfinite(old), fin), "non-finite entries differ between the flavours"
            assert fin.mean() > 0.9, "the inputs of this test are meant to stay finite (%d of %d entries are not)" % ((~fin).sum(), fin.size)
            for group, cols in (("X", slice(1, 1 + S)), ("u", slice(1 + S, 1 + S + NU)), ("H", slice(1 + S + NU, 2 + S + NU))):
                f = fin[:, cols]
                e_new = float(np.max(np.abs(new[:, cols][f] - ref[:, cols][f])))
                e_old = float(np.max(np.abs(old[:, cols][f] - ref[:, cols][f])))
                bar = 2.0 * e_old + 16.0 * EPS * float(np.max(np.abs(ref[:, cols][f])))
                print("fast %s stride %d %s form, %s: e_new %.3e  e_old %.3e  bar %.3e  (non-finite entries: %d of %d)"
                      % (name, stride, form, group, e_new, e_old, bar, (~f).sum(), f.size))
                if not e_new <= bar:
                    failures.append((stride, form, group, e_new, e_old, bar))
    ctx.close()
    assert not failures, failures


def test_fast_flavour_goddard():
    def make():
        ctx, prob, z = goddard_ctx("fast")
        return ctx, prob.mode_t, perturbed(z, 11, rel=0.002)
    fast_flavour_check("goddard", make, 14, 3)


def test_fast_flavour_vtol():
    fast_flavour_check("vtolUAV", lambda: vtol_ctx("fast"), 12, 3)


def test_argument_errors_empty_batch_and_counters(goddard_case):
    from socp_amd import capi
    ctx, prob, Z, full = goddard_case
    W = ctx.trace_width()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    Zc = np.ascontiguousarray(Z)
    rows, count = np.zeros(11 * 6 * 4 * W), np.zeros(66, dtype=np.int32)
    args = lambda B, stride, cap: (ctx.h, B, Zc.ctypes.data_as(dp), stride, cap, rows.ctypes.data_as(dp), count.ctypes.data_as(ip))  # noqa: E731
    t0, l0 = ctx.counters()
    for B, stride, cap in ((11, 0, 4), (11, -1, 4), (11, 1, 0), (-1, 1, 4)):
        assert ctx.L.socp_trace_batch(*args(B, stride, cap)) == capi.ERR_ARG, (B, stride, cap)
        assert ctx.L.socp_trace_batch_dev(ctx.h, B, None, stride, cap, None, None) == capi.ERR_ARG, (B, stride, cap)
    assert ctx.L.socp_trace_batch(*args(0, 1, 4)) == capi.OK and ctx.L.socp_trace_batch_dev(ctx.h, 0, None, 1, 4, None, None) == capi.OK
    assert ctx.counters() == (t0, l0)                   # nothing was launched
    assert ctx.L.socp_trace_batch(*args(11, 4, 4)) == capi.OK
    t1, l1 = ctx.counters()
    assert t1 - t0 == 11 * 6 and l1 - l0 == 2           # B M trajectories; the integration launch and the u / H launch
    fresh = capi.Context(capi.MODEL_GODDARD)
    assert fresh.L.socp_trace_batch(fresh.h, 1, Zc.ctypes.data_as(dp), 1, 4, rows.ctypes.data_as(dp), count.ctypes.data_as(ip)) == capi.ERR_ARG
    assert "no problem set" in fresh.L.socp_last_error(fresh.h).decode()
    assert fresh.trace_width() == W
    fresh.close()


def test_trace_of_converged_chains_ends_where_the_trajectory_batch_ends():
    """After chains_solve of 64 KD chains: trace_batch of the solutions with the chains' final parameter blocks -- the last kept
    X of every segment is socp_integrate_batch of that segment, bit for bit."""
    from socp_amd import capi, sweep
    ctx = capi.Context(capi.MODEL_GODDARD)
    ctx.set_params(sweep.GODDARD_PARAMS)
    ctx.set_step_number(10)
    P, M, s = 64, 6, 14
    Z0, params, goals, kd = sweep.goddard_kd_chains(ctx, P)
    res = ctx.chains_solve(Z0, kind=capi.CHAIN_PARAM, param_index=kd, step=1.0, goal=goals, params=params, xtol=1e-8)
    assert np.sum(res["info"] == 1) >= P // 2
    blocks = np.concatenate([params, np.zeros((P, 2))], axis=1)
    blocks[:, kd] = res["param_final"]
    rows, count = ctx.trace_batch(res["z"], stride=10, params=blocks)
    assert np.all(count == 2)
    for p in range(P):
        ctx.set_params(blocks[p, :8])
        tl = ctx.timeline(res["z"][p])
        Xf = ctx.integrate_batch(tl[:M], tl[1:], res["z"][p, :s * M].reshape(M, s))
        assert np.array_equal(u64(rows[p, :, 1, 1:1 + s]), u64(Xf)), p
        assert np.array_equal(u64(rows[p, :, 0, 1:1 + s]), u64(res["z"][p, :s * M].reshape(M, s))), p
    ctx.close()
