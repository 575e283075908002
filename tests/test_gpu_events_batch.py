"""GPU: the batched event location (socp_events_batch[_dev] / _blocks, capi.Context.events_batch) against
tests/events_reference.py -- the definition restated in numpy on the CPU oracle's RK4 step.  Outputs live in sentinel-filled
buffers followed by 64 guard words and are compared WHOLE on integer views (the conventions of test_gpu_cost_batch.py), so a
store past a slab, past min(count, cap) or through a NULL Xev shows.  The inputs are tests/events_cases.py; test_events_cpu.py
checks on the CPU that every channel stays > 1e-6 away from its levels at every step end, so the event SETS of the two
flavours must agree exactly.
Exact flavour: t, id, count and Xev bit-equal to the reference.  Throughput flavour: id and count equal, the event times within
FAST_BOUND of the CPU reference's relative to the segment length; the figures the test prints are kept in
profiles/events_gpu_tests.txt."""
import ctypes as C
import os

import numpy as np
import pytest

import events_cases as ec
from events_reference import pack_events

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0x7FF8DEADBEEF0001                       # a NaN no kernel produces
SENT_I = 0x5EADBEE1                             # no event id, no count
GUARD = 64
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
# |t_fast - t_reference| / segment length.  The project's bar for the throughput flavour is 1e-8; the bound is ten times the
# largest figure measured over all cases of test 5 (profiles/events_gpu_tests.txt), and never looser than that bar.
FAST_MEASURED = 2.488e-13                       # goddard_b130, R = 2, on an MI355X
FAST_BOUND = 1e-8 if FAST_MEASURED is None else min(10.0 * FAST_MEASURED, 1e-8)


def sentinel(size):
    return np.full(size + GUARD, np.uint64(SENT), dtype=np.uint64).view(np.float64)


def sentinel_i(size):
    return np.full(size + GUARD, SENT_I, dtype=np.int32)


def context(name, variant="exact"):
    """A context set to a case: model, parameters, step number, problem."""
    from socp_amd import capi
    c = ec.case(name)
    ctx = capi.Context({"goddard": capi.MODEL_GODDARD, "dint": capi.MODEL_DOUBLE_INTEGRATOR, "covid": capi.MODEL_COVID19}[c["model"]])
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    ctx.set_params(c["params"])
    ctx.set_step_number(c["N"])
    prob = c["prob"]
    assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == prob.n
    return ctx, c


# ---- the three forms on guarded buffers: each returns the four WHOLE buffers (tev, id, count, Xev) as integer views ----------

def buffers(B, M, cap, s):
    return sentinel(B * M * cap), sentinel_i(B * M * cap), sentinel_i(B * M), sentinel(B * M * cap * s)


def views(t, ident, count, X):
    return t.view(np.uint64), ident, count, X.view(np.uint64)


def run_host(ctx, c, R, cap, xev=True, blocks=None):
    Z, lv, ch = np.ascontiguousarray(c["Z"]), np.ascontiguousarray(c["levels"]), np.ascontiguousarray(c["chan"], dtype=np.int32)
    B = len(Z)
    t, ident, count, X = buffers(B, ctx.M, cap, ctx.s)
    tail = (len(ch), ch.ctypes.data_as(IP), lv.ctypes.data_as(DP), R, cap, t.ctypes.data_as(DP), ident.ctypes.data_as(IP),
            count.ctypes.data_as(IP), X.ctypes.data_as(DP) if xev else None)
    if blocks is None:
        ctx._chk(ctx.L.socp_events_batch(ctx.h, B, Z.ctypes.data_as(DP), *tail))
    else:
        pp, tt, xx = (np.ascontiguousarray(a) for a in blocks)
        ctx._chk(ctx.L.socp_events_batch_blocks(ctx.h, B, Z.ctypes.data_as(DP), pp.ctypes.data_as(DP), pp.shape[1], tt.ctypes.data_as(DP),
                                                xx.ctypes.data_as(DP), *tail))
    return views(t, ident, count, X)


def run_dev(ctx, c, R, cap, xev=True, blocks=None):
    import torch
    B = len(c["Z"])
    up = lambda a: torch.from_numpy(np.array(a)).cuda()        # noqa: E731  (a copy: the cases' arrays are read-only)
    dZ, dL = up(c["Z"]), up(c["levels"])
    dT, dI, dC, dX = (up(a) for a in buffers(B, ctx.M, cap, ctx.s))
    keep = [up(a) for a in blocks] if blocks is not None else []
    if blocks is not None:
        ctx._chk(ctx.L.socp_problem_set_blocks_dev(ctx.h, keep[0].data_ptr(), blocks[0].shape[1], keep[1].data_ptr(), keep[2].data_ptr()))
    torch.cuda.synchronize()
    try:
        ctx.events_batch_dev(B, dZ.data_ptr(), c["chan"], dL.data_ptr(), R, cap, dT.data_ptr(), dI.data_ptr(), dC.data_ptr(),
                             dX.data_ptr() if xev else None)
        ctx.synchronize()
        torch.cuda.synchronize()
    finally:
        if blocks is not None:
            ctx.L.socp_problem_set_blocks_dev(ctx.h, None, 0, None, None)
    return views(*(a.cpu().numpy() for a in (dT, dI, dC, dX)))


def expected(name, R, cap, xev=True):
    """What a form must leave in sentinel-filled buffers: the four arrays of pack_events (Xev None: nothing may be written)."""
    c = ec.case(name)
    return pack_events(ec.reference(name, R), cap, 2 * c["prob"].dim, fill_bits=SENT, fill_id=SENT_I, xev=xev)


def check_whole(got, want, what):
    fills = (np.uint64(SENT), SENT_I, SENT_I, np.uint64(SENT))
    for name, g, w, fill in zip(("tev", "id", "count", "Xev"), got, want, fills):
        if w is None:
            assert np.all(g == fill), "%s: %s was written although its pointer was NULL" % (what, name)
            continue
        w = np.ascontiguousarray(w).ravel()
        w = w.view(np.uint64) if w.dtype == np.float64 else w
        assert np.all(g[w.size:] == fill), "%s: guard words behind %s were written" % (what, name)
        bad = np.argwhere(g[:w.size] != w).ravel()
        assert len(bad) == 0, (what, name, "first differing flat indices:", bad[:5].tolist(), g[:w.size][bad[:5]], w[bad[:5]])


# ---- 1. exact flavour, bit for bit: host, _dev and _blocks forms, R = 0 and R = 2 -------------------------------------------

@pytest.mark.parametrize("R", [0, 2])
@pytest.mark.parametrize("name", ["goddard_b130", "goddard_n100"])
def test_goddard_bit_for_bit(name, R):
    ctx, c = context(name)
    assert ctx.event_channels() == 1
    want = expected(name, R, cap=4)
    assert want[2].max() == 2 and want[2].sum() >= 2 * len(c["Z"]), "every row has events, some segments two"
    check_whole(run_host(ctx, c, R, 4), want, "%s R = %d, host form" % (name, R))
    check_whole(run_dev(ctx, c, R, 4), want, "%s R = %d, _dev form" % (name, R))
    ctx.close()


def test_golden_row_events_are_the_cpu_s():
    """Row 0 of the batch is the golden stage-3 row: the two events test_events_cpu.py pins on the shooting timeline."""
    ctx, c = context("goddard_b130")
    t, ident, count = ctx.events_batch(c["Z"][:1], c["chan"], [-0.4, 0.0], refine=2)
    assert count[0].tolist() == [1, 0, 0, 1, 0, 0] and ident[0, 0, 0] == 1 and ident[0, 3, 0] == 2
    assert t[0, 0, 0] == 0.005012714637908262 and t[0, 3, 0] == 0.11913872605795653
    ctx.close()


@pytest.mark.parametrize("R", [0, 2])
def test_blocks_form_with_a_level_per_row(R):
    """mu2, hence the saturation level, the initial time and the node table differ from row to row: _blocks, and
    socp_problem_set_blocks_dev + _dev with socp_problem_blocks_all_smooth 0 and 1."""
    name = "goddard_blocks"
    ctx, c = context(name)
    want = expected(name, R, cap=4)
    check_whole(run_host(ctx, c, R, 4, blocks=c["blocks"]), want, "_blocks form, R = %d" % R)
    # _blocks restores the context's own blocks: the shared-parameter call afterwards is the plain one
    plain = run_host(ctx, c, R, 4)
    assert not np.array_equal(plain[0][:want[0].size], want[0].ravel().view(np.uint64))
    for smooth in (0, 1):
        ctx._chk(ctx.L.socp_problem_blocks_all_smooth(ctx.h, smooth))
        check_whole(run_dev(ctx, c, R, 4, blocks=c["blocks"]), want, "set_blocks_dev + _dev, all_smooth = %d, R = %d" % (smooth, R))
    ctx._chk(ctx.L.socp_problem_blocks_all_smooth(ctx.h, 0))
    again = run_host(ctx, c, R, 4)
    assert all(np.array_equal(a, b) for a, b in zip(plain, again))
    ctx.close()


# ---- 2. cap and NULL Xev --------------------------------------------------------------------------------------------------

def test_cap_one_counts_all_and_stores_one_and_null_xev_is_not_written():
    name = "goddard_b130"
    ctx, c = context(name)
    want = expected(name, 2, cap=1)
    assert want[2].max() == 2, "rows with two events in one segment"
    for run, form in ((run_host, "host form"), (run_dev, "_dev form")):
        check_whole(run(ctx, c, 2, 1), want, "cap = 1, " + form)
        check_whole(run(ctx, c, 2, 1, xev=False), want[:3] + (None,), "cap = 1, NULL Xev, " + form)
        check_whole(run(ctx, c, 2, 4, xev=False), expected(name, 2, 4)[:3] + (None,), "cap = 4, NULL Xev, " + form)
    # the Python form calls again with the largest count
    t, ident, count, X = ctx.events_batch(c["Z"], c["chan"], c["levels"], refine=2, cap=1, xev=True)
    full = pack_events(ec.reference(name, 2), 2, 14)
    assert t.shape[2] == 2 and np.array_equal(count, full[2])
    stored = ~np.isnan(full[0])
    assert np.array_equal(t[stored], full[0][stored]) and np.array_equal(ident[stored], full[1][stored]) and np.array_equal(X[stored], full[3][stored])
    assert np.all(np.isnan(t[~stored])) and np.all(ident[~stored] == 0)
    ctx.close()


# ---- 3. degenerate segments ---------------------------------------------------------------------------------------------

def test_zero_length_and_backward_segments_have_no_events():
    name = "goddard_degenerate"
    ctx, c = context(name)
    want = expected(name, 2, cap=3)
    assert np.all(want[2][:, 1:3] == 0) and np.all(want[2][:, 0] >= 1)
    for run, form in ((run_host, "host form"), (run_dev, "_dev form")):
        got = run(ctx, c, 2, 3)
        check_whole(got, want, "degenerate segments, " + form)
        assert np.all(got[2][:12].reshape(3, 4)[:, 1:3] == 0)
    ctx.close()


# ---- 4. the other two models ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["dint_basic", "covid_m20"])
def test_double_integrator_and_covid_bit_for_bit(name):
    ctx, c = context(name)
    assert ctx.event_channels() == (2 if name == "covid_m20" else 1)
    for R in (0, 2):
        rows = ec.reference(name, R)
        for e in range(len(c["chan"])):
            assert sum(1 for row in rows for seg in row for ev in seg if ev["e"] == e) >= 1, "the reference finds an event per watched channel"
        want = expected(name, R, cap=3)
        check_whole(run_host(ctx, c, R, 3), want, "%s R = %d, host form" % (name, R))
        check_whole(run_dev(ctx, c, R, 3), want, "%s R = %d, _dev form" % (name, R))
    ctx.close()


# ---- 5. throughput flavour ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["goddard_b130", "goddard_n100", "goddard_blocks", "dint_basic", "covid_m20"])
def test_fast_flavour_same_events_times_within_the_bound(name):
    """id and count equal to the exact flavour's (= the reference's, tests 1 and 4); max |t_fast - t_reference| / segment length
    printed and held against FAST_BOUND.  profiles/events_gpu_tests.txt keeps the figures."""
    from oracle.oracle import Problem
    ctx, c = context(name, "fast")
    B, M, cap = len(c["Z"]), ctx.M, 4
    worst = 0.0
    for R in (0, 2):
        want = expected(name, R, cap)
        got = run_dev(ctx, c, R, cap, blocks=c["blocks"])
        n = B * M * cap
        assert np.array_equal(got[1][:n], want[1].ravel()) and np.array_equal(got[2][:B * M], want[2].ravel()), "id and count are the exact flavour's"
        assert np.all(got[1][n:] == SENT_I) and np.all(got[2][B * M:] == SENT_I), "guard words behind id / count"
        assert np.all(got[0][n:] == np.uint64(SENT)) and np.all(got[3][n * ctx.s:] == np.uint64(SENT)), "guard words behind tev / Xev"
        stored = want[1] != SENT_I
        assert np.all(got[0][:n].reshape(B, M, cap)[~stored] == np.uint64(SENT)), "the slots beyond count are untouched"
        t = got[0][:n].view(np.float64).reshape(B, M, cap)
        blocks = c["blocks"] or (None, None, None)
        prob = c["prob"]
        dev = 0.0
        for b in range(B):
            pb = prob if blocks[1] is None else Problem(prob.dim, prob.mode_t, prob.mode_x, blocks[1][b], prob.xnode)
            tl = c["o"].timeline(pb, c["Z"][b])
            for i in range(M):
                k = stored[b, i]
                if k.any():
                    dev = max(dev, float(np.max(np.abs(t[b, i][k] - want[0][b, i][k]))) / abs(tl[i + 1] - tl[i]))
        print("fast %s R = %d: %d events, max |t_fast - t_ref| / segment length = %.3e (bound %.1e)" % (name, R, int(stored.sum()), dev, FAST_BOUND))
        worst = max(worst, dev)
    ctx.close()
    assert worst <= FAST_BOUND, worst


# ---- 6. errors; 7. counters ---------------------------------------------------------------------------------------------------

def raw_call(ctx, B, Z, E, chan, lv, R, cap, out):
    ch = np.ascontiguousarray(chan if chan is not None else [], dtype=np.int32)
    return ctx.L.socp_events_batch(ctx.h, B, Z.ctypes.data_as(DP) if Z is not None else None, E, ch.ctypes.data_as(IP) if chan is not None else None,
                                   lv.ctypes.data_as(DP) if lv is not None else None, R, cap, out[0].ctypes.data_as(DP), out[1].ctypes.data_as(IP),
                                   out[2].ctypes.data_as(IP), out[3].ctypes.data_as(DP))


def test_errors_leave_the_context_unchanged_and_counters():
    from socp_amd import capi
    name = "goddard_n100"
    ctx, c = context(name)
    Z, lv = np.ascontiguousarray(c["Z"]), np.ascontiguousarray(c["levels"])
    B, M = len(Z), ctx.M
    out = buffers(B, M, 4, ctx.s)
    fresh_out = lambda: all(np.all(a.view(np.uint64 if a.dtype == np.float64 else np.int32) == f)      # noqa: E731
                            for a, f in zip(out, (np.uint64(SENT), SENT_I, SENT_I, np.uint64(SENT))))
    L, h = ctx.L, ctx.h
    t0, l0 = ctx.counters()
    pb0 = ctx.timeline(Z[0]).copy()
    for E, chan, R, cap, what in ((0, [0, 0], 2, 4, "E = 0"), (9, [0] * 9, 2, 4, "E = 9"), (2, [0, 1], 2, 4, "channel 1 of 1"),
                                  (2, [-1, 0], 2, 4, "channel -1"), (2, [0, 0], 9, 4, "refine = 9"), (2, [0, 0], -1, 4, "refine = -1"),
                                  (2, [0, 0], 2, 0, "cap = 0")):
        assert raw_call(ctx, B, Z, E, chan, lv, R, cap, out) == capi.ERR_ARG, what
    assert raw_call(ctx, -1, Z, 2, [0, 0], lv, 2, 4, out) == capi.ERR_ARG
    assert raw_call(ctx, B, None, 2, [0, 0], lv, 2, 4, out) == capi.ERR_ARG and raw_call(ctx, B, Z, 2, [0, 0], None, 2, 4, out) == capi.ERR_ARG
    assert raw_call(ctx, B, Z, 2, None, lv, 2, 4, out) == capi.ERR_ARG
    ch = np.zeros(2, dtype=np.int32)
    assert L.socp_events_batch_dev(h, B, None, 2, ch.ctypes.data_as(IP), None, 2, 4, None, None, None, None) == capi.ERR_ARG
    params = np.tile(np.concatenate([ctx.get_params(), [0.0, 0.0]]), (B, 1))
    for stride in (8, 9, 11):
        assert L.socp_events_batch_blocks(h, B, Z.ctypes.data_as(DP), params.ctypes.data_as(DP), stride, None, None, 2, ch.ctypes.data_as(IP),
                                          lv.ctypes.data_as(DP), 2, 4, out[0].ctypes.data_as(DP), out[1].ctypes.data_as(IP),
                                          out[2].ctypes.data_as(IP), out[3].ctypes.data_as(DP)) == capi.ERR_ARG, stride
    assert "nparams + 2" in L.socp_last_error(h).decode()
    # B = 0: SOCP_OK and no launch
    assert raw_call(ctx, 0, None, 2, [0, 0], None, 2, 4, out) == capi.OK
    assert L.socp_events_batch_dev(h, 0, None, 2, ch.ctypes.data_as(IP), None, 2, 4, None, None, None, None) == capi.OK
    # the adaptive integrator
    ctx.set_integrator(capi.INT_DOPRI5, 1e-8)
    assert raw_call(ctx, B, Z, 2, [0, 0], lv, 2, 4, out) == capi.ERR_UNSUPPORTED and "DOPRI5" in L.socp_last_error(h).decode()
    assert L.socp_events_batch_dev(h, B, Z.ctypes.data_as(DP), 2, ch.ctypes.data_as(IP), lv.ctypes.data_as(DP), 2, 4, out[0].ctypes.data_as(DP),
                                   out[1].ctypes.data_as(IP), out[2].ctypes.data_as(IP), None) == capi.ERR_UNSUPPORTED      # refused before anything is enqueued
    ctx.set_integrator(capi.INT_RK4)
    assert ctx.counters() == (t0, l0), "nothing was launched or counted"
    assert fresh_out(), "nothing was written"
    assert np.array_equal(ctx.timeline(Z[0]), pb0)

    fresh = capi.Context(capi.MODEL_GODDARD)
    assert fresh.event_channels() == 1
    assert raw_call(fresh, B, Z, 2, [0, 0], lv, 2, 4, out) == capi.ERR_ARG and "no problem set" in fresh.L.socp_last_error(fresh.h).decode()
    fresh.close()

    # models without the trait: the interceptor (its own ComputeTraj) and the example plugin
    from test_gpu_interceptor import multi_shooting_problem, scenario_state
    from oracle.oracle import Oracle, MODEL_INTERCEPTOR
    Xs, Xf = scenario_state(gamma=1.49)
    iprob, iz = multi_shooting_problem(Oracle(MODEL_INTERCEPTOR), 4, X0=Xs, Xf=Xf)
    for variant in (capi.VARIANT_LANE_EXACT, capi.VARIANT_LANE_FAST):
        ci = capi.Context(capi.MODEL_INTERCEPTOR)
        ci.set_variant(variant)
        assert ci.problem_set(iprob.mode_t, iprob.mode_x, iprob.time, iprob.xnode) == iprob.n
        assert ci.event_channels() == 0
        c0 = ci.counters()
        io = buffers(1, 4, 4, 12)
        assert raw_call(ci, 1, np.ascontiguousarray(iz), 1, [0], np.zeros(1), 2, 4, io) == capi.ERR_UNSUPPORTED
        assert "no events entry" in ci.L.socp_last_error(ci.h).decode() and ci.counters() == c0
        with pytest.raises(capi.SocpError):
            ci.events_batch(iz[None, :], [0], [0.0])
        ci.close()
    from test_gpu_cost_batch import build_lqr1d
    p, _, Zp, _ = build_lqr1d()
    assert p.event_channels() == 0
    c0 = p.counters()
    po = buffers(len(Zp), p.M, 4, p.s)
    assert raw_call(p, len(Zp), np.ascontiguousarray(Zp), 1, [0], np.zeros(len(Zp)), 2, 4, po) == capi.ERR_UNSUPPORTED
    assert "no events entry" in p.L.socp_last_error(p.h).decode() and p.counters() == c0
    p.close()

    # a valid call afterwards reproduces test 1's bits; the counters advance by B M trajectories and ONE launch
    check_whole(run_host(ctx, c, 2, 4), expected(name, 2, 4), "after the refused calls")
    t1, l1 = ctx.counters()
    assert t1 - t0 == B * M and l1 - l0 == 1
    check_whole(run_dev(ctx, c, 0, 4, xev=False), expected(name, 0, 4)[:3] + (None,), "_dev form afterwards")
    t2, l2 = ctx.counters()
    assert t2 - t1 == B * M and l2 - l1 == 1
    ctx.close()
