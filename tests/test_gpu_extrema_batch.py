"""GPU: the batched extrema (socp_extrema_batch[_dev / _blocks], capi.Context.extrema_batch) against the restatement of
tests/extrema_reference.py applied to socp_trace_batch with stride = 1 ON THE SAME CONTEXT: the sequential reduction over the rows
the trace keeps, the event channels restated from the rows' states (tests/events_reference.py).  Reference-order flavour: every
output bit-equal, compared on uint64 / int32 views of the WHOLE caller buffers -- pre-filled with a NaN no kernel produces and
followed by guard words -- so a write into a column that is not selected, into a buffer that was not passed or outside [b][i]
fails; host and _dev form.  Throughput flavour (fixed step, Goddard and vtolUAV): values only, per channel group
e_new = max|extrema_fast - extrema_exact| within 2 e_old + 16 ulp of the group's largest magnitude, e_old the deviation of the same
reduction over the fast context's own stride-1 trace -- the rule of test_gpu_cost_batch.py: two independent contractions of the same
arithmetic.  The times of a flat channel are rounding noise there and are not compared; count must be equal.
Shapes: the smallest at which the kernel can still go wrong (390 lanes = rows straddling wavefronts and a partial last one).
Measured on an MI355X (profiles/extrema_gpu_tests.txt): e_new = e_old to three digits in every group but Goddard's event channel --
Goddard X 1.7e-6 (vmax; vmin 1.9e-9), u 1.6e-14, H 1.7e-6, g 1.289e-6 against 1.293e-6 (vmin; vmax 3.6e-15 against 1.1e-16, bar
9.6e-14); vtolUAV X 7.1e-15, u 4.1e-15, H 4.2e-17."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import extrema_reference as er
from test_gpu_trace_batch import goddard_ctx, perturbed, vtol_ctx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
EPS = 2.0 ** -52
ALL = 7


# ---- the forms on guarded buffers: each returns the six WHOLE buffers (vmin, vmax, tmin, tmax as uint64; count, nbad) ------------

def buffers(ctx, B):
    n = B * ctx.M * ctx.extrema_width()
    return [er.sentinel(n) for _ in range(4)] + [er.sentinel_i(B * ctx.M), er.sentinel_i(B * ctx.M)]


def views(bufs):
    return tuple(a.view(np.uint64) if a.dtype == np.float64 else a for a in bufs)


def run_host(ctx, Z, what, times=(True, True), nbad=True, blocks=None):
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    B = len(Z)
    lo, hi, ta, tb, cnt, bad = bufs = buffers(ctx, B)
    d = lambda a, on=True: a.ctypes.data_as(DP) if on else None      # noqa: E731
    tail = (what, d(lo), d(hi), d(ta, times[0]), d(tb, times[1]), cnt.ctypes.data_as(IP), bad.ctypes.data_as(IP) if nbad else None)
    if blocks is None:
        ctx._chk(ctx.L.socp_extrema_batch(ctx.h, B, d(Z), *tail))
    else:
        from socp_amd import capi
        ctx._chk(ctx.L.socp_extrema_batch_blocks(ctx.h, B, d(Z), *capi._block_args(B, *blocks), *tail))
    return views(bufs)


def run_dev(ctx, Z, what, times=(True, True), nbad=True, blocks=None):
    import torch
    B = len(Z)
    dZ = torch.from_numpy(np.array(Z, dtype=np.float64)).cuda()
    dev = [torch.from_numpy(a).cuda() for a in buffers(ctx, B)]
    held = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda() if a is not None else None for a in (blocks or ())]
    ptr = lambda t, on=True: t.data_ptr() if (on and t is not None) else None      # noqa: E731
    if blocks is not None:
        ctx._chk(ctx.L.socp_problem_set_blocks_dev(ctx.h, ptr(held[0]), blocks[0].shape[1] if blocks[0] is not None else 0, ptr(held[1]), ptr(held[2])))
    torch.cuda.synchronize()
    try:
        ctx.extrema_batch_dev(B, dZ.data_ptr(), what, ptr(dev[0]), ptr(dev[1]), ptr(dev[2], times[0]), ptr(dev[3], times[1]), ptr(dev[4]),
                              ptr(dev[5], nbad))
        ctx.synchronize()
        torch.cuda.synchronize()
    finally:
        if blocks is not None:
            ctx.L.socp_problem_set_blocks_dev(ctx.h, None, 0, None, None)
    return views([t.cpu().numpy() for t in dev])


NAMES = ("vmin", "vmax", "tmin", "tmax", "count", "nbad")


def check_whole(got, want, label):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape, (label, name)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (label, name, "first differing words:", bad[:6].tolist(), g[bad[:6]].tolist(), w[bad[:6]].tolist())


def trace_of(ctx, Z, blocks=None):
    """The rows socp_trace_batch keeps with stride = 1 on this context: (rows[B][M][cap][W], count[B][M]), every row stored."""
    p, t, x = blocks if blocks is not None else (None, None, None)
    rows, count = ctx.trace_batch(Z, stride=1, params=p, time=t, xnode=x)
    assert count.max() <= rows.shape[2]
    return rows, count


def reference(ctx, Z, what, model=None, blocks=None, trace=None):
    """The restatement over the context's own stride-1 trace: list [b][i] (extrema_reference.reference_extrema)."""
    rows, count = trace if trace is not None else trace_of(ctx, Z, blocks)
    event, EC = er.EVENT_FN[model] if model else (None, 0)
    assert ctx.extrema_width() == ctx.s + ctx.nu + 1 + EC and ctx.event_channels() == EC
    params = None
    if EC:
        params = blocks[0][:, :-2] if (blocks is not None and blocks[0] is not None) else ctx.get_params()
    return er.reference_from_trace(rows, count, ctx.s, ctx.nu, what, event, EC, params)


def both_forms_bit_equal(ctx, Z, whats, model=None, blocks=None, label=""):
    trace = trace_of(ctx, Z, blocks)
    refs = {}
    for what in whats:
        refs[what] = reference(ctx, Z, what, model, blocks, trace)
        want = er.pack_extrema(refs[what])
        check_whole(run_host(ctx, Z, what, blocks=blocks), want, "%s what %d, host form" % (label, what))
        check_whole(run_dev(ctx, Z, what, blocks=blocks), want, "%s what %d, _dev form" % (label, what))
    return refs


# ---- Goddard, M = 3 (free tf, n = 43), N = 10, B = 130: 390 lanes -----------------------------------------------------------------

def goddard_m3(variant="exact", mu2=1.0, step_nbr=10):
    from socp_amd import capi
    ctx, prob, z = goddard_ctx(variant, mu2=mu2, step_nbr=step_nbr)
    mode_t = [capi.FIXED, capi.CONTINUOUS, capi.CONTINUOUS, capi.FREE]
    mode_x = np.zeros((4, 7), dtype=np.int32)
    mode_x[1:3] = capi.CONTINUOUS
    mode_x[3, 3:7] = capi.FREE
    pick = [0, 2, 4, 6]
    assert ctx.problem_set(mode_t, mode_x, prob.time[pick], prob.xnode[pick]) == 43
    z3 = np.concatenate([prob.xnode[[0, 2, 4]].ravel(), [prob.time[6]]])
    return ctx, (mode_t, mode_x, prob.time[pick], prob.xnode[pick]), z3


@pytest.fixture(scope="module")
def goddard_case():
    ctx, problem, z3 = goddard_m3()
    Z = perturbed(z3, 130, rel=0.002)
    Z.setflags(write=False)
    trace = trace_of(ctx, Z)
    yield ctx, Z, trace
    ctx.close()


@pytest.mark.parametrize("what", [0, 2, 7])
def test_goddard_390_lanes_bit_equal_host_and_dev(goddard_case, what):
    ctx, Z, trace = goddard_case
    assert ctx.extrema_width() == 14 + 3 + 1 + 1 and ctx.has_extrema()
    ref = reference(ctx, Z, what, "goddard", trace=trace)
    assert all(r["count"] == 11 for row in ref for r in row)
    want = er.pack_extrema(ref)
    check_whole(run_host(ctx, Z, what), want, "host form")
    check_whole(run_dev(ctx, Z, what), want, "_dev form")
    if what == 7:
        # the figure the feature is for, through the Python layer: the spread of H along a row
        r = ctx.extrema_batch(Z)
        assert r["channels"][17] == "H" and r["channels"][18] == "g0" and len(r["channels"]) == 19
        assert np.array_equal(er.u64(r["vmin"]).ravel(), want[0][:r["vmin"].size]) and np.array_equal(r["count"].ravel(), want[4][:390])
        spread = r["vmax"][:, :, 17].max(axis=1) - r["vmin"][:, :, 17].min(axis=1)
        print("goddard M = 3, N = 10, 130 perturbed rows: H spread along a row %.3e .. %.3e" % (spread.min(), spread.max()))
        assert np.all(spread >= 0.0)
    if what == 0:
        r = ctx.extrema_batch(Z, what=0)
        assert np.all(np.isnan(r["vmin"][:, :, 14:])) and np.all(np.isfinite(r["vmin"][:, :, :14]))


@pytest.mark.parametrize("times,nbad", [((False, False), False), ((True, False), True), ((False, True), False)])
def test_goddard_null_tmin_tmax_nbad(goddard_case, times, nbad):
    ctx, Z, trace = goddard_case
    want = er.pack_extrema(reference(ctx, Z, ALL, "goddard", trace=trace), times=times, nbad=nbad)
    check_whole(run_host(ctx, Z, ALL, times, nbad), want, "host form")
    check_whole(run_dev(ctx, Z, ALL, times, nbad), want, "_dev form")


def test_goddard_bang_singular_off_switch_inside_a_segment():
    """mu2 = 0: the control law reads the switching times, placed INSIDE segments of the M = 6 layout; then FREE interior times,
    whose switching times come from z."""
    from socp_amd import capi
    ctx, prob, z = goddard_ctx(mu2=0.0)
    Z = perturbed(z, 3, rel=0.01)
    tl = ctx.timeline(Z[0])
    ctx.set_switching_times([0.5 * (tl[1] + tl[2]), 0.5 * (tl[3] + tl[4])])
    refs = both_forms_bit_equal(ctx, Z, [ALL, 1], "goddard", label="context switching times")
    thrust = np.array([[np.abs(r["vmax"][14:17]).max() for r in row] for row in refs[ALL]])
    assert np.all(thrust[:, 0] > 0.0) and np.all(thrust[:, 5] == 0.0), "bang before the first switch, off after the second"
    mode_t = [capi.FIXED, capi.FREE, capi.FREE, capi.FREE]
    mode_x = np.zeros((4, 7), dtype=np.int32)
    mode_x[1:3] = capi.CONTINUOUS
    mode_x[3, 3:7] = capi.FREE
    assert ctx.problem_set(mode_t, mode_x, prob.time[[0, 2, 4, 6]], prob.xnode[[0, 2, 4, 6]]) == 45
    ctx.set_param("singularControl", -1.0)
    z3 = np.concatenate([prob.xnode[[0, 2, 4]].ravel(), prob.time[[2, 4, 6]]])
    both_forms_bit_equal(ctx, perturbed(z3, 4, rel=0.01, seed=11), [ALL], "goddard", label="switching times from z")
    ctx.close()


def test_goddard_per_row_blocks_each_row_equal_to_the_row_alone():
    """B = 70, N = 7: every row with its own KD and mu2, initial time and node states.  Against the restatement over the trace with
    the same blocks (whole buffers, host and _dev form), and row by row against the call on a context set to that row alone."""
    ctx, problem, z3 = goddard_m3(step_nbr=7)
    mode_t, mode_x, time0, xnode0 = problem
    B = 70
    Z = perturbed(z3, B, rel=0.01, seed=3)
    base = np.concatenate([ctx.get_params(), [0.0, 0.0]])
    params = np.tile(base, (B, 1))
    params[:, 2] = np.linspace(0.0, 400.0, B)
    params[:, 6] = np.linspace(0.5, 1.5, B)
    time = np.tile(time0, (B, 1))
    time[:, 0] = 1e-3 * np.sin(np.arange(B))
    xnode = np.tile(xnode0.ravel(), (B, 1)) * (1.0 + 1e-3 * np.arange(B))[:, None]
    blocks = (params, time, xnode)
    refs = both_forms_bit_equal(ctx, Z, [ALL, 0], "goddard", blocks=blocks, label="blocks")     # 0: the state-only kernel under blocks
    got = run_host(ctx, Z, ALL, blocks=blocks)
    assert ctx.get_params().tolist() == base[:8].tolist(), "the context's own parameters are back in force"
    Cw, M = ctx.extrema_width(), 3
    for b in range(B):
        ctx.set_params(params[b, :8])
        ctx.set_switching_times(params[b, 8:])
        ctx.problem_set(mode_t, mode_x, time[b], xnode[b].reshape(4, 14))
        alone = run_host(ctx, Z[b:b + 1], ALL)
        for name, g, a in zip(NAMES, got, alone):
            w = M * Cw if g.dtype == np.uint64 else M
            assert np.array_equal(g[b * w:(b + 1) * w], a[:w]), (b, name)
    assert len({r["vmax"][17] for row in refs[ALL] for r in row}) > B, "the rows differ"
    ctx.close()


def test_zero_length_and_backward_segments_have_one_row():
    from socp_amd import capi
    ctx, prob, z = goddard_ctx()
    mode_t = [capi.FIXED] * 5
    mode_x = np.zeros((5, 7), dtype=np.int32)
    mode_x[1:4] = capi.CONTINUOUS
    t = np.array([0.0, 0.02, 0.02, 0.015, 0.04])          # segment 1 has zero length, segment 2 runs backward
    assert ctx.problem_set(mode_t, mode_x, t, prob.xnode[:5]) == 56
    Z = perturbed(prob.xnode[:4].ravel(), 3, seed=5)
    refs = both_forms_bit_equal(ctx, Z, [ALL, 0], "goddard", label="degenerate segments")
    for b in range(3):
        assert [r["count"] for r in refs[ALL][b]] == [11, 1, 1, 11]
        for i in (1, 2):
            r = refs[ALL][b][i]
            assert np.array_equal(er.u64(r["vmin"]), er.u64(r["vmax"])) and np.all(r["tmin"] == t[i]) and np.all(r["tmax"] == t[i])
            assert np.array_equal(er.u64(r["vmin"][:14]), er.u64(Z[b, 14 * i:14 * i + 14]))
    ctx.close()


def test_a_nan_start_state_stays_in_its_own_lane(goddard_case):
    ctx, Z, trace = goddard_case
    Zn = np.array(Z[:5])
    Zn[2, 14 + 3] = np.nan                                 # v_x at the start of segment 1 of row 2
    refs = both_forms_bit_equal(ctx, Zn, [ALL, 0], "goddard", label="NaN start")
    r = refs[ALL][2][1]
    assert r["nbad"] == r["count"] == 11 and np.isnan(r["vmin"][3]) and r["tmin"][3] == r["tmax"][3]
    assert refs[0][2][1]["nbad"] == 11 and refs[ALL][2][0]["nbad"] == 0 and refs[ALL][2][2]["nbad"] == 0
    got, clean = run_host(ctx, Zn, ALL), run_host(ctx, Z[:5], ALL)
    Cw = ctx.extrema_width()
    lane = 2 * 3 + 1
    for name, g, c in zip(NAMES, got, clean):
        w = Cw if g.dtype == np.uint64 else 1
        keep = np.ones(len(g), dtype=bool)
        keep[lane * w:(lane + 1) * w] = False
        assert np.array_equal(g[keep], c[keep]), "the neighbours of the NaN lane changed: " + name


# ---- the double integrator (M = 1) and covid19 (M = 20): event channels included ---------------------------------------------------

@pytest.mark.parametrize("name", ["dint_basic", "covid_m20"])
def test_dint_and_covid_with_their_event_channels(name):
    import events_cases as ec
    from socp_amd import capi
    c = ec.case(name)
    ctx = capi.Context({"dint": capi.MODEL_DOUBLE_INTEGRATOR, "covid": capi.MODEL_COVID19}[c["model"]])
    ctx.set_params(c["params"])
    ctx.set_step_number(c["N"])
    prob = c["prob"]
    assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == prob.n
    EC = {"dint": 1, "covid": 2}[c["model"]]
    assert ctx.extrema_width() == ctx.s + ctx.nu + 1 + EC
    refs = both_forms_bit_equal(ctx, c["Z"], [ALL, 4, 3], c["model"], label=name)
    assert all(r["count"] == c["N"] + 1 and r["nbad"] == 0 for row in refs[ALL] for r in row)
    if c["model"] == "covid":
        # channel 1 is the state I = X[2]: the same extrema, bit for bit
        for row in refs[ALL]:
            for r in row:
                assert np.array_equal(er.u64(r["vmax"][-1:]), er.u64(r["vmax"][2:3])) and r["tmax"][-1] == r["tmax"][2]
    ctx.close()


# ---- plugins, the adaptive integrator, the interceptor, vtolUAV ------------------------------------------------------------------------

def test_osc1d_plugin_and_adaptive_integrator_on_goddard_and_the_plugin():
    import jacobi_cases as jc
    from test_gpu_jacobi_batch import context
    from socp_amd import capi
    c = jc.case("osc1d")
    p = context(c)
    assert p.has_extrema() and p.event_channels() == 0 and p.extrema_width() == 2 + 1 + 1
    refs = both_forms_bit_equal(p, c["Z"], [ALL, 0], label="osc1d")
    assert all(r["count"] == c["N"] + 1 for row in refs[ALL] for r in row)
    p.set_integrator(capi.INT_DOPRI5, 1e-8)
    refs = both_forms_bit_equal(p, c["Z"], [ALL], label="osc1d adaptive")
    counts = {r["count"] for row in refs[ALL] for r in row}
    print("adaptive osc1d: rows per segment %d .. %d" % (min(counts), max(counts)))
    p.close()

    ctx, prob, z = goddard_ctx()
    ctx.set_integrator(capi.INT_DOPRI5, 1e-8)
    Z = perturbed(z, 11, rel=0.002)
    Z[:, -1] = z[-1] * np.linspace(0.5, 2.0, 11)           # free tf: segments from short to long
    refs = both_forms_bit_equal(ctx, Z, [ALL, 0], "goddard", label="goddard adaptive")
    counts = [r["count"] for row in refs[ALL] for r in row]
    print("adaptive goddard: rows per segment %d .. %d" % (min(counts), max(counts)))
    assert len(set(counts[:64])) > 1, "lanes of one wave end with different numbers of rows"
    ctx.close()


@pytest.mark.parametrize("adaptive", [False, True])
def test_interceptor_counts_the_extra_final_row(adaptive):
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
        Xs, Xf = scenario_state(gamma=1.49)               # |cos(gamma)| < chartLimit: starts with a chart change
        prob, z = multi_shooting_problem(o, 4, X0=Xs, Xf=Xf)
    ctx = capi.Context(capi.MODEL_INTERCEPTOR)
    ctx.set_step_number(6)
    if adaptive:
        ctx.set_integrator(capi.INT_DOPRI5, 1e-8)
    assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == prob.n
    assert ctx.extrema_width() == 12 + 2 + 1 and ctx.event_channels() == 0
    Z = np.tile(z, (2, 1))
    Z[1, 6:12] *= 1.0 + 1e-3
    refs = both_forms_bit_equal(ctx, Z, [ALL, 0], label="interceptor")
    counts = [r["count"] for r in refs[ALL][0]]
    print("interceptor %s: rows per segment %s" % ("adaptive" if adaptive else "fixed step", counts))
    if not adaptive:
        assert counts == [8, 8, 8, 15]                      # stage start + 6 steps + the extra final row; the last segment crosses t1 = 20 s
    ctx.close()


def test_vtol_with_the_synthetic_obstacle_map():
    ctx, mode_t, Z = vtol_ctx("exact")
    assert ctx.extrema_width() == 12 + 3 + 1 and ctx.event_channels() == 0
    refs = both_forms_bit_equal(ctx, Z, [ALL, 0], label="vtolUAV")
    assert all(r["count"] == 9 for row in refs[ALL] for r in row)
    ctx.close()


# ---- throughput flavour: the fast context's own trace is the yardstick ---------------------------------------------------------------

def fast_flavour_check(name, ctx, Z, model, S, NU, EC):
    from socp_amd import capi
    ctx.set_variant(capi.VARIANT_LANE_EXACT)
    exact = run_dev(ctx, Z, ALL)
    check_whole(exact, er.pack_extrema(reference(ctx, Z, ALL, model)), name + ": the exact side")
    ctx.set_variant(capi.VARIANT_LANE_FAST)
    old = er.pack_extrema(reference(ctx, Z, ALL, model))             # the same reduction over the fast context's stride-1 trace
    failures = []
    n = len(Z) * ctx.M * (S + NU + 1 + EC)
    groups = [("X", slice(0, S)), ("u", slice(S, S + NU)), ("H", slice(S + NU, S + NU + 1))] + ([("g", slice(S + NU + 1, S + NU + 1 + EC))] if EC else [])
    for form, new in (("host", run_host(ctx, Z, ALL)), ("dev", run_dev(ctx, Z, ALL))):
        assert np.array_equal(new[4], exact[4]) and np.array_equal(old[4], exact[4]), "count"
        assert np.array_equal(new[5], exact[5]), "nbad"
        for k in range(4):
            assert np.all(new[k][n:] == er.SENT), "guard words"
        for side, k in (("vmin", 0), ("vmax", 1)):
            a, b, ref = (v[k][:n].view(np.float64).reshape(-1, S + NU + 1 + EC) for v in (new, old, exact))
            assert np.all(np.isfinite(ref)) and np.all(np.isfinite(a)), "the inputs of this test are meant to stay finite"
            for group, cols in groups:
                e_new = float(np.max(np.abs(a[:, cols] - ref[:, cols])))
                e_old = float(np.max(np.abs(b[:, cols] - ref[:, cols])))
                bar = 2.0 * e_old + 16.0 * EPS * float(np.max(np.abs(ref[:, cols])))
                print("fast %s %s form, %s of %s: e_new %.3e  e_old %.3e  bar %.3e" % (name, form, side, group, e_new, e_old, bar))
                if not e_new <= bar:
                    failures.append((form, side, group, e_new, e_old, bar))
    ctx.close()
    assert not failures, failures


def test_fast_flavour_goddard():
    ctx, problem, z3 = goddard_m3("fast")
    fast_flavour_check("goddard", ctx, perturbed(z3, 22, rel=0.002), "goddard", 14, 3, 1)


def test_fast_flavour_vtol():
    ctx, mode_t, Z = vtol_ctx("fast")
    fast_flavour_check("vtolUAV", ctx, Z, None, 12, 3, 0)


# ---- surface ---------------------------------------------------------------------------------------------------------------------------

def test_argument_errors_write_nothing_empty_batch_and_counters(goddard_case):
    from socp_amd import capi
    ctx, Z, trace = goddard_case
    B, M, Cw = 4, 3, ctx.extrema_width()
    Zc = np.ascontiguousarray(Z[:B])
    wrong_stride = np.zeros((B, 8 + 2 + 1))              # Goddard: nparams + 2 = 10

    def call(form, B_=B, what=ALL, Zp=Zc, null=(), blocks=None):
        """One call on sentinel-filled buffers (device buffers for the _dev form); returns the code after checking that nothing was written."""
        import torch
        bufs = buffers(ctx, B)
        if form == "_dev":
            held = [torch.from_numpy(a).cuda() for a in bufs]
            zd = torch.from_numpy(np.array(Zp)).cuda() if Zp is not None else None
            p = [t.data_ptr() for t in held]
            zp = zd.data_ptr() if zd is not None else None
            torch.cuda.synchronize()
        else:
            p = [a.ctypes.data_as(DP) for a in bufs[:4]] + [a.ctypes.data_as(IP) for a in bufs[4:]]
            zp = Zp.ctypes.data_as(DP) if Zp is not None else None
        for k in null:
            p[k] = None
        if form == "blocks":
            rc = ctx.L.socp_extrema_batch_blocks(ctx.h, B_, zp, blocks.ctypes.data_as(DP), blocks.shape[1], None, None, what, *p)
        else:
            rc = getattr(ctx.L, "socp_extrema_batch" + form)(ctx.h, B_, zp, what, *p)
        if form == "_dev":
            ctx.synchronize()
            torch.cuda.synchronize()
            bufs = [t.cpu().numpy() for t in held]
        for a in bufs:
            assert np.all(a.view(np.uint64 if a.dtype == np.float64 else np.int32) == (er.SENT if a.dtype == np.float64 else er.SENT_I)), "an error wrote"
        return rc
    t0, l0 = ctx.counters()
    for form in ("", "_dev"):
        assert call(form, B_=-1) == capi.ERR_ARG
        assert call(form, what=8) == capi.ERR_ARG and call(form, what=-1) == capi.ERR_ARG
        assert call(form, Zp=None) == capi.ERR_ARG
        for k in (0, 1, 4):                 # vmin, vmax, count
            assert call(form, null=(k,)) == capi.ERR_ARG, k
        assert call(form, B_=0) == capi.OK and call(form, B_=0, Zp=None, null=(0, 1, 2, 3, 4, 5)) == capi.OK
    assert call("blocks", blocks=wrong_stride) == capi.ERR_ARG and "stride" in ctx.L.socp_last_error(ctx.h).decode()
    assert call("blocks", B_=-1, blocks=wrong_stride[:, :-1]) == capi.ERR_ARG
    assert ctx.counters() == (t0, l0), "a refused or empty call counted"
    fresh = capi.Context(capi.MODEL_GODDARD)
    bufs = buffers(ctx, 1)
    assert fresh.L.socp_extrema_batch(fresh.h, 1, Zc.ctypes.data_as(DP), ALL, *[a.ctypes.data_as(DP) for a in bufs[:4]],
                                      *[a.ctypes.data_as(IP) for a in bufs[4:]]) == capi.ERR_ARG
    assert "no problem set" in fresh.L.socp_last_error(fresh.h).decode()
    fresh.close()
    for what, form in ((ALL, run_host), (0, run_host), (ALL, run_dev), (2, run_dev)):
        a, b = ctx.counters()
        form(ctx, Zc, what)
        c, d = ctx.counters()
        assert (c - a, d - b) == (B * M, 1), (what, form.__name__)


def test_widths_of_the_five_in_tree_models():
    from socp_amd import capi
    want = {capi.MODEL_GODDARD: 14 + 3 + 1 + 1, capi.MODEL_DOUBLE_INTEGRATOR: 12 + 3 + 1 + 1, capi.MODEL_COVID19: 8 + 1 + 1 + 2,
            capi.MODEL_INTERCEPTOR: 12 + 2 + 1 + 0, capi.MODEL_VTOLUAV: 12 + 3 + 1 + 0}
    for model, width in want.items():
        ctx = capi.Context(model)
        assert ctx.extrema_width() == width and ctx.has_extrema() and len(ctx.extrema_channels()) == width, model
        assert ctx.L.socp_extrema_width(None) == capi.ERR_ARG and ctx.L.socp_ctx_has_extrema(None) == capi.ERR_ARG
        ctx.close()


def test_sweep_tool_writes_the_extrema_file_and_record(tmp_path):
    out = str(tmp_path / "ext")
    run = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--starts", "64", "--rk4-steps", "50", "--extrema-out", out], cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    entry = rec["extrema"]
    assert {"rows", "h_spread_max", "h_spread_median", "nbad_rows"} <= set(entry)
    npz = np.load(entry["file"])
    assert entry["file"] == out + ".rank0.npz" and sorted(npz.files) == sorted(["index", "vmin", "vmax", "tmin", "tmax", "count", "nbad"])
    k = entry["rows"]
    assert k == rec["converged"] == len(npz["index"]) > 0
    assert npz["vmin"].shape == (k, 1, 19) and np.all(npz["count"] == 51) and npz["nbad"].shape == (k, 1)
    spread = npz["vmax"][:, :, 17].max(axis=1) - npz["vmin"][:, :, 17].min(axis=1)
    print("sweep of 64 starts, N = 50: H spread max %.3e median %.3e" % (entry["h_spread_max"], entry["h_spread_median"]))
    assert entry["h_spread_max"] == float(spread.max()) and entry["h_spread_median"] == float(np.median(spread)) and spread.min() >= 0.0
    assert entry["nbad_rows"] == int(np.sum(npz["nbad"].sum(axis=1) > 0)) == 0
    assert np.all(npz["vmin"] <= npz["vmax"]) and np.all(npz["tmin"] >= 0.0)
    bad = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--extrema-out", out, "--extrema-what", "8"], cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--extrema-what" in bad.stderr
