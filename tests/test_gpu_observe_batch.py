"""GPU: the batched observables (socp_observe_batch[_dev / _blocks], capi.Context.observe_batch) against the restatement of
tests/observe_reference.py applied to socp_trace_batch with stride = 1 ON THE SAME CONTEXT: every in-tree model's observables and
the osc1d_observe plugin's restated from the rows' (t, X, u), then the sequential reduction -- extrema under strict comparisons,
the composite trapezoid, the count of rows that are not finite.  Reference-order flavour: every output bit-equal, compared on
uint64 / int32 views of the WHOLE caller buffers -- pre-filled with a NaN no kernel produces and followed by guard words -- so a
write into a buffer that was not passed or outside [b][i] fails; host, _dev and _blocks forms.
Throughput flavour (fixed step, Goddard and vtolUAV): per observable, e_old = the largest deviation over ALL rows of the observable
restated on the fast context's own stride-1 trace from the one restated on the reference-order trace; the bar of the extrema tests,
2 e_old + 16 ulp of the observable's largest magnitude, holds ymin and ymax of the fast call against the reference-order call, and
that bar times the segment's length holds the integrals (a trapezoid sum of row values that each move by at most the bar).  The
times of a flat observable are rounding noise there and are not compared.  clearance is never contracted: its ymin, ymax, tmin and
tmax are bit-equal to the restatement over the fast trace, and so are count and nbad.
Shapes: the smallest at which the kernel can still go wrong (210 lanes = rows straddling wavefronts and a partial last one).
Measured on an MI355X (profiles/observe_gpu_tests.txt): every reference-order comparison bit-equal; throughput flavour, largest
e_new / bar: Goddard 0.90 (ymax of drag: 7.1e-13 against 7.9e-13), its integrals 0.31; vtolUAV 0.28 (norm_u), its integrals 0.05;
clearance bit-equal.  The stored testVtolUAV flow's converged solutions: smallest clearance 5.5 (one waypoint) falling to 1.31 at 32
waypoints -- they do not graze an obstacle."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import observe_reference as obr
from test_gpu_trace_batch import goddard_ctx, perturbed
from test_gpu_extrema_batch import goddard_m3

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
EPS = 2.0 ** -52
NAMES = ("ymin", "ymax", "tmin", "tmax", "integral", "count", "nbad")
ALL3 = (True, True, True)
OSC1D_OBSERVE_ID = 1006
VP_ALPHAV, VP_CA, VP_PHIOBS = 3, 6, 9                      # models_vtol.hpp: VtolParam


@pytest.fixture(scope="module", autouse=True)
def _plugin_built():
    """tests/conftest.py rebuilds only when an artefact IT lists is missing; a tree built before this plugin existed lacks it."""
    if not os.path.exists(plugin_path()):
        import __graft_entry__
        __graft_entry__.build()
    return True


def plugin_path(name="osc1d_observe"):
    return os.path.join(ROOT, "socp_amd", "_build", "plugins", "lib%s_plugin.so" % name)


# ---- the forms on guarded buffers: each returns the seven WHOLE buffers (five as uint64; count, nbad) --------------------------------

def width(ctx):
    return len(ctx.observable_names())


def buffers(ctx, B, NO=None):
    n = B * ctx.M * (width(ctx) if NO is None else NO)
    return [obr.sentinel(n) for _ in range(5)] + [obr.sentinel_i(B * ctx.M), obr.sentinel_i(B * ctx.M)]


def views(bufs):
    return tuple(a.view(np.uint64) if a.dtype == np.float64 else a for a in bufs)


def run_host(ctx, Z, given=ALL3, nbad=True, blocks=None):
    """socp_observe_batch, or socp_observe_batch_blocks when blocks = (params, time, xnode) is given."""
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    B = len(Z)
    lo, hi, ta, tb, ig, cnt, bad = bufs = buffers(ctx, B)
    d = lambda a, on=True: a.ctypes.data_as(DP) if on else None      # noqa: E731
    tail = (d(lo), d(hi), d(ta, given[0]), d(tb, given[1]), d(ig, given[2]), cnt.ctypes.data_as(IP), bad.ctypes.data_as(IP) if nbad else None)
    if blocks is None:
        ctx._chk(ctx.L.socp_observe_batch(ctx.h, B, d(Z), *tail))
    else:
        from socp_amd import capi
        ctx._chk(ctx.L.socp_observe_batch_blocks(ctx.h, B, d(Z), *capi._block_args(B, *blocks), *tail))
    return views(bufs)


def run_dev(ctx, Z, given=ALL3, nbad=True, blocks=None):
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
        ctx.observe_batch_dev(B, dZ.data_ptr(), ptr(dev[0]), ptr(dev[1]), ptr(dev[2], given[0]), ptr(dev[3], given[1]), ptr(dev[4], given[2]),
                              ptr(dev[5]), ptr(dev[6], nbad))
        ctx.synchronize()
        torch.cuda.synchronize()
    finally:
        if blocks is not None:
            ctx.L.socp_problem_set_blocks_dev(ctx.h, None, 0, None, None)
    return views([t.cpu().numpy() for t in dev])


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


def reference(ctx, Z, model, blocks=None, trace=None, table=None):
    """The restatement over the context's own stride-1 trace: list [b][i] (observe_reference.reduce_rows)."""
    rows, count = trace if trace is not None else trace_of(ctx, Z, blocks)
    assert ctx.has_observe() and ctx.observable_names() == obr.OBSERVE[model][3]
    params = blocks[0][:, :-2] if (blocks is not None and blocks[0] is not None) else ctx.get_params()
    return obr.reference_from_trace(model, rows, count, params, table)


def all_forms_bit_equal(ctx, Z, model, blocks=None, table=None, label=""):
    ref = reference(ctx, Z, model, blocks, table=table)
    want = obr.pack_observe(ref)
    check_whole(run_host(ctx, Z, blocks=blocks), want, label + ", host form")
    check_whole(run_dev(ctx, Z, blocks=blocks), want, label + ", _dev form")
    return ref


# ---- Goddard, M = 3 (free tf, n = 43), N = 20, B = 70: 210 lanes -------------------------------------------------------------------

@pytest.fixture(scope="module")
def goddard_case():
    ctx, problem, z3 = goddard_m3(step_nbr=20)
    Z = perturbed(z3, 70, rel=0.002)
    Z.setflags(write=False)
    ref = reference(ctx, Z, "goddard")
    yield ctx, Z, ref
    ctx.close()


def test_goddard_210_lanes_bit_equal_host_dev_and_blocks(goddard_case):
    ctx, Z, ref = goddard_case
    assert ctx.observable_names() == ["r", "v", "norm_u", "drag", "drag_acc", "fuel_rate"] and ctx.has_observe()
    assert all(r["count"] == 21 and r["nbad"] == 0 for row in ref for r in row)
    want = obr.pack_observe(ref)
    check_whole(run_host(ctx, Z), want, "host form")
    check_whole(run_dev(ctx, Z), want, "_dev form")
    # the _blocks form with every row's block equal to the context's own: the same bits through the per-row kernel
    own = np.tile(np.concatenate([ctx.get_params(), [0.0, 0.0]]), (len(Z), 1))
    check_whole(run_host(ctx, Z, blocks=(own, None, None)), want, "_blocks form")
    check_whole(run_dev(ctx, Z, blocks=(own, None, None)), want, "blocks in force, _dev form")
    # through the Python layer, and the figures the feature is for
    r = ctx.observe_batch(Z)
    assert r["names"] == ctx.observable_names() and r["ymin"].shape == (70, 3, 6)
    for k, key in enumerate(NAMES[:5]):
        assert np.array_equal(obr.u64(r[key]).ravel(), want[k][:r[key].size]), key
    assert np.array_equal(r["count"].ravel(), want[5][:210]) and np.array_equal(r["nbad"].ravel(), want[6][:210])
    burnt = r["integral"][:, :, 5].sum(axis=1)
    print("goddard M = 3, N = 20, 70 perturbed rows: peak drag %.4e .. %.4e, burnt fuel (integral of fuel_rate) %.4e .. %.4e, peak r %.6f"
          % (r["ymax"][:, :, 3].max(axis=1).min(), r["ymax"][:, :, 3].max(), burnt.min(), burnt.max(), r["ymax"][:, :, 0].max()))
    assert np.all(burnt > 0.0) and np.all(r["ymin"][:, :, 3] >= 0.0)


@pytest.mark.parametrize("B", [1, 63, 64, 65])
def test_goddard_sub_batches_equal_the_same_rows_of_the_70(goddard_case, B):
    ctx, Z, ref = goddard_case
    want = obr.pack_observe(ref[:B])
    check_whole(run_host(ctx, Z[:B]), want, "host form, B = %d" % B)
    check_whole(run_dev(ctx, Z[:B]), want, "_dev form, B = %d" % B)


@pytest.mark.parametrize("given,nbad", [((False, False, False), False), ((True, False, True), True), ((False, True, False), False),
                                        ((True, True, False), True)])
def test_goddard_null_tmin_tmax_integral_nbad(goddard_case, given, nbad):
    ctx, Z, ref = goddard_case
    want = obr.pack_observe(ref[:9], given=given, nbad=nbad)
    check_whole(run_host(ctx, Z[:9], given, nbad), want, "host form")
    check_whole(run_dev(ctx, Z[:9], given, nbad), want, "_dev form")


def test_goddard_bang_singular_off_switch_inside_a_segment():
    """mu2 = 0: the control law reads the switching times, placed INSIDE segments; then FREE interior times, whose switching times
    come from z."""
    from socp_amd import capi
    ctx, prob, z = goddard_ctx(mu2=0.0, step_nbr=20)
    Z = perturbed(z, 3, rel=0.01)
    tl = ctx.timeline(Z[0])
    ctx.set_switching_times([0.5 * (tl[1] + tl[2]), 0.5 * (tl[3] + tl[4])])
    ref = all_forms_bit_equal(ctx, Z, "goddard", label="context switching times")
    thrust = np.array([[r["ymax"][2] for r in row] for row in ref])
    assert np.all(thrust[:, 0] > 0.0) and np.all(thrust[:, 5] == 0.0), "bang before the first switch, off after the second"
    mode_t = [capi.FIXED, capi.FREE, capi.FREE, capi.FREE]
    mode_x = np.zeros((4, 7), dtype=np.int32)
    mode_x[1:3] = capi.CONTINUOUS
    mode_x[3, 3:7] = capi.FREE
    assert ctx.problem_set(mode_t, mode_x, prob.time[[0, 2, 4, 6]], prob.xnode[[0, 2, 4, 6]]) == 45
    ctx.set_param("singularControl", -1.0)
    z3 = np.concatenate([prob.xnode[[0, 2, 4]].ravel(), prob.time[[2, 4, 6]]])
    all_forms_bit_equal(ctx, perturbed(z3, 4, rel=0.01, seed=11), "goddard", label="switching times from z")
    ctx.close()


def test_goddard_per_row_blocks_each_row_equal_to_the_row_alone():
    """B = 24, N = 20: every row with its own KD, b and mu2, initial time and node states.  Against the restatement over the trace
    with the same blocks (whole buffers, host and _dev form), and row by row against the call on a context set to that row alone."""
    ctx, problem, z3 = goddard_m3(step_nbr=20)
    mode_t, mode_x, time0, xnode0 = problem
    B = 24
    Z = perturbed(z3, B, rel=0.01, seed=3)
    base = np.concatenate([ctx.get_params(), [0.0, 0.0]])
    params = np.tile(base, (B, 1))
    params[:, 1] = np.linspace(5.0, 9.0, B)
    params[:, 2] = np.linspace(0.0, 400.0, B)
    params[:, 6] = np.linspace(0.5, 1.5, B)
    time = np.tile(time0, (B, 1))
    time[:, 0] = 1e-3 * np.sin(np.arange(B))
    xnode = np.tile(xnode0.ravel(), (B, 1)) * (1.0 + 1e-3 * np.arange(B))[:, None]
    blocks = (params, time, xnode)
    ref = all_forms_bit_equal(ctx, Z, "goddard", blocks=blocks, label="blocks")
    got = run_host(ctx, Z, blocks=blocks)
    assert ctx.get_params().tolist() == base[:8].tolist(), "the context's own parameters are back in force"
    NO, M = 6, 3
    for b in range(B):
        ctx.set_params(params[b, :8])
        ctx.set_switching_times(params[b, 8:])
        ctx.problem_set(mode_t, mode_x, time[b], xnode[b].reshape(4, 14))
        alone = run_host(ctx, Z[b:b + 1])
        for name, g, a in zip(NAMES, got, alone):
            w = M * NO if g.dtype == np.uint64 else M
            assert np.array_equal(g[b * w:(b + 1) * w], a[:w]), (b, name)
    assert len({r["ymax"][3] for row in ref for r in row}) > B, "the rows differ"
    assert ref[0][0]["ymax"][3] == 0.0, "KD = 0: no drag"
    ctx.close()


def test_zero_length_and_backward_segments_have_one_row_and_a_zero_integral():
    from socp_amd import capi
    ctx, prob, z = goddard_ctx(step_nbr=20)
    mode_t = [capi.FIXED] * 5
    mode_x = np.zeros((5, 7), dtype=np.int32)
    mode_x[1:4] = capi.CONTINUOUS
    t = np.array([0.0, 0.02, 0.02, 0.015, 0.04])          # segment 1 has zero length, segment 2 runs backward
    assert ctx.problem_set(mode_t, mode_x, t, prob.xnode[:5]) == 56
    Z = perturbed(prob.xnode[:4].ravel(), 3, seed=5)
    ref = all_forms_bit_equal(ctx, Z, "goddard", label="degenerate segments")
    for b in range(3):
        assert [r["count"] for r in ref[b]] == [21, 1, 1, 21]
        for i in (1, 2):
            r = ref[b][i]
            assert np.array_equal(obr.u64(r["ymin"]), obr.u64(r["ymax"])) and np.all(r["tmin"] == t[i]) and np.all(r["tmax"] == t[i])
            assert np.array_equal(obr.u64(r["integral"]), obr.u64(np.zeros(6))), "+0.0"
    ctx.close()


def test_a_nan_start_state_stays_in_its_own_lane(goddard_case):
    ctx, Z, ref70 = goddard_case
    Zn = np.array(Z[:5])
    Zn[2, 14 + 3] = np.nan                                 # v_x at the start of segment 1 of row 2
    ref = all_forms_bit_equal(ctx, Zn, "goddard", label="NaN start")
    r = ref[2][1]
    assert r["nbad"] == r["count"] == 21 and np.isnan(r["ymin"][1]) and np.isnan(r["integral"][1]) and r["tmin"][1] == r["tmax"][1]
    assert ref[2][0]["nbad"] == 0 and ref[2][2]["nbad"] == 0
    got, clean = run_host(ctx, Zn), run_host(ctx, Z[:5])
    lane = 2 * 3 + 1
    for name, g, c in zip(NAMES, got, clean):
        w = 6 if g.dtype == np.uint64 else 1
        keep = np.ones(len(g), dtype=bool)
        keep[lane * w:(lane + 1) * w] = False
        assert np.array_equal(g[keep], c[keep]), "the neighbours of the NaN lane changed: " + name


def test_goddard_adaptive_integrator():
    from socp_amd import capi
    ctx, prob, z = goddard_ctx()
    ctx.set_integrator(capi.INT_DOPRI5, 1e-8)
    Z = perturbed(z, 11, rel=0.002)
    Z[:, -1] = z[-1] * np.linspace(0.5, 2.0, 11)           # free tf: segments from short to long
    ref = all_forms_bit_equal(ctx, Z, "goddard", label="goddard adaptive")
    counts = [r["count"] for row in ref for r in row]
    print("adaptive goddard: rows per segment %d .. %d" % (min(counts), max(counts)))
    assert len(set(counts[:64])) > 1, "lanes of one wave end with different numbers of rows"
    ctx.close()


# ---- vtolUAV, M = 4, N = 10 --------------------------------------------------------------------------------------------------------

def vtol_path4(variant="exact", table=None):
    """The four-waypoint stage of the stored flow (n = 52) at its converged solution, 10 steps per segment."""
    import test_gpu_vtol as tv
    from socp_amd import capi
    ctx = capi.Context(capi.MODEL_VTOLUAV)
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    table = tv.V["table_shipped"] if table is None else table
    ctx.set_map(table)
    _, _, zstar = tv.stage_problem(ctx, "path_4")
    ctx.set_step_number(10)
    assert ctx.M == 4 and ctx.observable_names() == ["speed", "norm_u", "clearance"]
    return ctx, np.array(table, dtype=np.float64), zstar


def test_vtol_shipped_map():
    ctx, table, zstar = vtol_path4()
    Z = np.concatenate([zstar[None, :], perturbed(zstar, 5, rel=0.01, seed=13)])
    ref = all_forms_bit_equal(ctx, Z, "vtol", table=table, label="vtolUAV shipped map")
    assert all(r["count"] == 11 and r["nbad"] == 0 for row in ref for r in row)
    print("vtolUAV path_4 at its converged solution, shipped map, N = 10: smallest clearance per segment %s"
          % ", ".join("%.4f" % r["ymin"][2] for r in ref[0]))
    ctx.close()


def test_vtol_coasting_path_through_a_box_has_negative_clearance():
    """A synthetic three-obstacle map and parameters under which a row with zero costates coasts on a straight line (phiObs = 0:
    no map gradient; ca = alphaV = 0: no drag, no speed term; zero costates: u = 0): row 0 is aimed at the centre of a box and
    passes through it in segment 0, row 1 passes 3 beside it; every other segment is the path beside."""
    table = np.array([[1.0, 10.0, 0.0, 5.0, 1.0, 1.0, 1.0],          # the box in the way
                      [0.0, 40.0, 40.0, 5.0, 2.0, 3.0, 4.0],         # an ellipsoid far off
                      [1.0, -30.0, 0.0, 5.0, 1.0, 2.0, 3.0]])        # a box behind
    ctx, table, zstar = vtol_path4(table=table)
    P = ctx.get_params()
    P[VP_PHIOBS], P[VP_CA], P[VP_ALPHAV] = 0.0, 0.0, 0.0
    ctx.set_params(P)
    beside = np.zeros(12)
    beside[:6] = [5.0, 3.0, 5.0, 5.0, 0.0, 0.0]
    through = beside.copy()
    through[1] = 0.0
    times = [1.0, 2.0, 3.0, 4.0]                             # FREE node times: every segment lasts 1, 5 along x
    Z = np.array([np.concatenate([through, beside, beside, beside, times]), np.concatenate([beside, beside, beside, beside, times])])
    assert Z.shape[1] == ctx.n == 52
    ref = all_forms_bit_equal(ctx, Z, "vtol", table=table, label="vtolUAV coasting")
    k = 2
    print("vtolUAV coasting rows: smallest clearance through the box %.4f at t = %.2f, beside it %.4f"
          % (ref[0][0]["ymin"][k], ref[0][0]["tmin"][k], ref[1][0]["ymin"][k]))
    assert ref[0][0]["ymin"][k] < 0.0 and abs(ref[0][0]["ymin"][k] + 1.0) < 1e-12 and ref[0][0]["tmin"][k] > 0.99, "row 0 ends at the box's centre"
    assert ref[0][0]["ymax"][k] == 4.0 and ref[0][0]["tmax"][k] == 0.0
    assert all(r["ymin"][k] > 0.0 for r in ref[1]) and all(r["ymin"][k] == 2.0 for r in ref[0][1:])
    assert all(r["ymax"][1] == 0.0 and r["ymin"][0] == 5.0 == r["ymax"][0] for row in ref for r in row), "u = 0 and a constant speed"
    ctx.close()


def test_vtol_256_obstacle_map_and_empty_map():
    fix = np.load(os.path.join(GOLD, "vtol_pin.npz"))
    ctx, table, zstar = vtol_path4(table=fix["table_grid256"])
    assert len(table) == 256
    Z = perturbed(zstar, 4, rel=0.01, seed=17)
    ref = all_forms_bit_equal(ctx, Z, "vtol", table=table, label="vtolUAV 256 obstacles")
    assert all(np.isfinite(r["ymin"][2]) for row in ref for r in row)
    ctx.set_map(np.zeros((0, 7)))
    ref = all_forms_bit_equal(ctx, Z, "vtol", table=np.zeros((0, 7)), label="vtolUAV empty map")
    for row in ref:
        for r in row:
            assert r["ymin"][2] == np.inf == r["ymax"][2] == r["integral"][2] and r["nbad"] == r["count"] == 11, "+inf is not finite"
    ctx.close()


def test_vtol_flow_converged_solutions_clearance():
    """The figure the feature is for: the smallest clearance along every converged solution of the stored testVtolUAV flow (shipped
    map, the stages' own parameters and step number), bit-equal to the restatement; printed, and recorded in
    profiles/observe_gpu_tests.txt.  Asserted: only that it is finite -- whether the scenario grazes an obstacle is a result."""
    import test_gpu_vtol as tv
    from socp_amd import capi
    ctx = capi.Context(capi.MODEL_VTOLUAV)
    ctx.set_map(tv.V["table_shipped"])
    smallest = {}
    for stage in ("path_1", "path_2", "path_4", "path_8", "path_16", "path_32", "invSigma", "muObs", "u_max"):
        _, _, zstar = tv.stage_problem(ctx, stage)
        r = ctx.observe_batch(zstar[None, :])
        k = r["names"].index("clearance")
        i = int(np.argmin(r["ymin"][0, :, k]))
        smallest[stage] = float(r["ymin"][0, i, k])
        print("vtolUAV flow stage %-8s (M = %2d): smallest clearance %.4f in segment %d at t = %.4f; peak speed %.4f, peak |u| %.4f, rows %d, nbad %d"
              % (stage, ctx.M, smallest[stage], i, r["tmin"][0, i, k], r["ymax"][0, :, 0].max(), r["ymax"][0, :, 1].max(),
                 int(r["count"].sum()), int(r["nbad"].sum())))
        if stage in ("path_4", "u_max"):
            check_whole(run_host(ctx, zstar[None, :]), obr.pack_observe(reference(ctx, zstar[None, :], "vtol", table=tv.V["table_shipped"])), stage)
    print("vtolUAV flow: smallest clearance over the flow %.4f (stage %s)" % (min(smallest.values()), min(smallest, key=smallest.get)))
    assert all(np.isfinite(v) for v in smallest.values())
    ctx.close()


# ---- the double integrator (M = 1), covid19 (M = 20), the plugin: both integrators ---------------------------------------------------

@pytest.mark.parametrize("name", ["dint_basic", "covid_m20"])
def test_dint_and_covid_both_integrators(name):
    import events_cases as ec
    from socp_amd import capi
    c = ec.case(name)
    ctx = capi.Context({"dint": capi.MODEL_DOUBLE_INTEGRATOR, "covid": capi.MODEL_COVID19}[c["model"]])
    ctx.set_params(c["params"])
    ctx.set_step_number(c["N"])
    prob = c["prob"]
    assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == prob.n
    assert ctx.observable_names() == {"dint": ["norm_u"], "covid": ["u"]}[c["model"]]
    ref = all_forms_bit_equal(ctx, c["Z"], c["model"], label=name)
    assert all(r["count"] == c["N"] + 1 and r["nbad"] == 0 for row in ref for r in row)
    if c["model"] == "covid":
        total = [sum(r["integral"][0] for r in row) for row in ref]
        print("covid19 M = 20: total intervention (integral of u over the segments) %.6f .. %.6f" % (min(total), max(total)))
    ctx.set_integrator(capi.INT_DOPRI5, 1e-8)
    ref = all_forms_bit_equal(ctx, c["Z"], c["model"], label=name + " adaptive")
    counts = [r["count"] for row in ref for r in row]
    print("adaptive %s: rows per segment %d .. %d" % (name, min(counts), max(counts)))
    ctx.close()


def osc1d_observe_ctx(N=20):
    import jacobi_cases as jc
    from socp_amd import capi
    c = jc.case("osc1d")
    capi.plugin_load(plugin_path())
    ctx = capi.Context(OSC1D_OBSERVE_ID, nparams=1)
    ctx.set_params(c["params"])
    ctx.set_step_number(N)
    prob = c["prob"]
    assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == prob.n
    return ctx, c["Z"]


def test_osc1d_observe_plugin_both_integrators():
    from socp_amd import capi
    ctx, Z = osc1d_observe_ctx()
    assert ctx.has_observe() and ctx.observable_names() == ["energy", "abs_u"]
    ref = all_forms_bit_equal(ctx, Z, "osc1d_observe", label="osc1d_observe")
    assert all(r["count"] == 21 and r["nbad"] == 0 for row in ref for r in row)
    ctx.set_integrator(capi.INT_DOPRI5, 1e-8)
    ref = all_forms_bit_equal(ctx, Z, "osc1d_observe", label="osc1d_observe adaptive")
    counts = {r["count"] for row in ref for r in row}
    print("adaptive osc1d_observe: rows per segment %d .. %d" % (min(counts), max(counts)))
    ctx.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def refused(ctx, Z, NO=2):
    """A model without the entry: UNSUPPORTED with the message, nothing written, the counters unchanged -- every form."""
    import torch
    from socp_amd import capi
    assert not ctx.has_observe() and ctx.observable_names() == [] and ctx.L.socp_ctx_observables(ctx.h) == 0
    assert ctx.L.socp_ctx_observable_name(ctx.h, 0) is None
    Z = np.array(Z, dtype=np.float64)
    B = len(Z)
    before = ctx.counters()
    bufs = buffers(ctx, B, NO)
    p = [a.ctypes.data_as(DP) for a in bufs[:5]] + [a.ctypes.data_as(IP) for a in bufs[5:]]
    assert ctx.L.socp_observe_batch(ctx.h, B, Z.ctypes.data_as(DP), *p) == capi.ERR_UNSUPPORTED
    assert "no observe entry" in ctx.L.socp_last_error(ctx.h).decode()
    assert ctx.L.socp_observe_batch_blocks(ctx.h, B, Z.ctypes.data_as(DP), None, 0, None, None, *p) == capi.ERR_UNSUPPORTED
    assert "no observe entry" in ctx.L.socp_last_error(ctx.h).decode()
    held = [torch.from_numpy(a).cuda() for a in bufs]
    dZ = torch.from_numpy(Z).cuda()
    torch.cuda.synchronize()
    assert ctx.L.socp_observe_batch_dev(ctx.h, B, dZ.data_ptr(), *[t.data_ptr() for t in held]) == capi.ERR_UNSUPPORTED
    assert "no observe entry" in ctx.L.socp_last_error(ctx.h).decode()
    ctx.synchronize()
    torch.cuda.synchronize()
    for a in bufs + [t.cpu().numpy() for t in held]:
        assert np.all(a.view(np.uint64 if a.dtype == np.float64 else np.int32) == (obr.SENT if a.dtype == np.float64 else obr.SENT_I)), "a refusal wrote"
    assert ctx.counters() == before, "a refused call counted"
    with pytest.raises(Exception):
        ctx.observe_batch(Z)


@pytest.mark.parametrize("variant", ["exact", "fast"])
def test_interceptor_is_refused(variant):
    from socp_amd import capi
    from oracle.oracle import Oracle, MODEL_INTERCEPTOR
    from test_gpu_interceptor import multi_shooting_problem, scenario_state
    o = Oracle(MODEL_INTERCEPTOR)
    Xs, Xf = scenario_state(gamma=1.49)
    prob, z = multi_shooting_problem(o, 4, X0=Xs, Xf=Xf)
    ctx = capi.Context(capi.MODEL_INTERCEPTOR)
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    ctx.set_step_number(6)
    assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == prob.n
    refused(ctx, np.tile(z, (2, 1)))
    assert ctx.has_extrema(), "what the interceptor had before stays"
    ctx.close()


def test_lqr1d_is_refused_and_a_valid_call_follows():
    import jacobi_cases as jc
    from test_gpu_jacobi_batch import context
    c = jc.case("lqr1d")
    p = context(c)
    refused(p, c["Z"])
    p.close()
    for name in ("osc1d",):                                 # the existing osc1d plugins stay without the trait
        q = context(jc.case(name))
        assert not q.has_observe()
        q.close()
    ctx, Z = osc1d_observe_ctx()
    all_forms_bit_equal(ctx, Z[:3], "osc1d_observe", label="after the refusals")
    ctx.close()


# ---- surface ----------------------------------------------------------------------------------------------------------------------

def test_argument_errors_write_nothing_empty_batch_and_counters(goddard_case):
    from socp_amd import capi
    ctx, Z, ref = goddard_case
    B, M = 4, 3
    Zc = np.ascontiguousarray(Z[:B])
    wrong_stride = np.zeros((B, 8 + 2 + 1))              # Goddard: nparams + 2 = 10

    def call(form, B_=B, Zp=Zc, null=(), blocks=None):
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
            p = [a.ctypes.data_as(DP) for a in bufs[:5]] + [a.ctypes.data_as(IP) for a in bufs[5:]]
            zp = Zp.ctypes.data_as(DP) if Zp is not None else None
        for k in null:
            p[k] = None
        if form == "blocks":
            rc = ctx.L.socp_observe_batch_blocks(ctx.h, B_, zp, blocks.ctypes.data_as(DP), blocks.shape[1], None, None, *p)
        else:
            rc = getattr(ctx.L, "socp_observe_batch" + form)(ctx.h, B_, zp, *p)
        if form == "_dev":
            ctx.synchronize()
            torch.cuda.synchronize()
            bufs = [t.cpu().numpy() for t in held]
        for a in bufs:
            assert np.all(a.view(np.uint64 if a.dtype == np.float64 else np.int32) == (obr.SENT if a.dtype == np.float64 else obr.SENT_I)), "an error wrote"
        return rc
    t0, l0 = ctx.counters()
    for form in ("", "_dev"):
        assert call(form, B_=-1) == capi.ERR_ARG
        assert call(form, Zp=None) == capi.ERR_ARG
        for k in (0, 1, 5):                 # ymin, ymax, count
            assert call(form, null=(k,)) == capi.ERR_ARG, k
        assert call(form, B_=0) == capi.OK and call(form, B_=0, Zp=None, null=(0, 1, 2, 3, 4, 5, 6)) == capi.OK
    assert call("blocks", blocks=wrong_stride) == capi.ERR_ARG and "stride" in ctx.L.socp_last_error(ctx.h).decode()
    assert call("blocks", B_=-1, blocks=wrong_stride[:, :-1]) == capi.ERR_ARG
    assert ctx.counters() == (t0, l0), "a refused or empty call counted"
    fresh = capi.Context(capi.MODEL_GODDARD)
    bufs = buffers(ctx, 1)
    assert fresh.L.socp_observe_batch(fresh.h, 1, Zc.ctypes.data_as(DP), *[a.ctypes.data_as(DP) for a in bufs[:5]],
                                      *[a.ctypes.data_as(IP) for a in bufs[5:]]) == capi.ERR_ARG
    assert "no problem set" in fresh.L.socp_last_error(fresh.h).decode()
    assert fresh.L.socp_ctx_has_observe(None) == capi.ERR_ARG and fresh.L.socp_ctx_observables(None) == capi.ERR_ARG
    assert fresh.L.socp_ctx_observable_name(fresh.h, 6) is None and fresh.L.socp_ctx_observable_name(fresh.h, -1) is None
    assert fresh.L.socp_ctx_observable_name(fresh.h, 5) == b"fuel_rate"
    fresh.close()
    for form in (run_host, run_dev):
        a, b = ctx.counters()
        form(ctx, Zc)
        c, d = ctx.counters()
        assert (c - a, d - b) == (B * M, 1), form.__name__


# ---- throughput flavour: the fast context's own trace is the yardstick -------------------------------------------------------------

def fast_flavour_check(name, ctx, Z, model, table=None, unfused=()):
    from socp_amd import capi
    NO = width(ctx)
    ctx.set_variant(capi.VARIANT_LANE_EXACT)
    trace_exact = trace_of(ctx, Z)
    exact = run_dev(ctx, Z)
    check_whole(exact, obr.pack_observe(reference(ctx, Z, model, trace=trace_exact, table=table)), name + ": the exact side")
    ctx.set_variant(capi.VARIANT_LANE_FAST)
    trace_fast = trace_of(ctx, Z)
    assert np.array_equal(trace_fast[1], trace_exact[1]), "fixed step: the same rows"
    old = obr.pack_observe(reference(ctx, Z, model, trace=trace_fast, table=table))     # the restatement over the fast context's rows
    params = ctx.get_params()
    B, M = trace_exact[1].shape
    e_old, mag, length = np.zeros(NO), np.zeros(NO), np.zeros(B * M)
    for b in range(B):
        for i in range(M):
            R = trace_exact[1][b, i]
            te, Ye = obr.observables_of_rows(model, trace_exact[0][b, i, :R], params, table)
            tf, Yf = obr.observables_of_rows(model, trace_fast[0][b, i, :R], params, table)
            assert np.all(np.isfinite(Ye)) and np.all(np.isfinite(Yf)), "the inputs of this test are meant to stay finite"
            e_old = np.maximum(e_old, np.max(np.abs(Yf - Ye), axis=0))
            mag = np.maximum(mag, np.max(np.abs(Ye), axis=0))
            length[b * M + i] = abs(te[-1] - te[0])
    bar = 2.0 * e_old + 16.0 * EPS * mag
    n = B * M * NO
    failures = []
    names = ctx.observable_names()
    for form, new in (("host", run_host(ctx, Z)), ("dev", run_dev(ctx, Z))):
        assert np.array_equal(new[5], exact[5]) and np.array_equal(new[5], old[5]), "count"
        assert np.array_equal(new[6], exact[6]) and np.array_equal(new[6], old[6]), "nbad"
        for k in range(5):
            assert np.all(new[k][n:] == obr.SENT), "guard words"
        for c in unfused:                   # never contracted: the bits of the restatement over the fast context's own rows
            for k in range(4):
                assert np.array_equal(new[k][:n].reshape(-1, NO)[:, c], old[k][:n].reshape(-1, NO)[:, c]), (names[c], NAMES[k])
        for side, k in (("ymin", 0), ("ymax", 1), ("integral", 4)):
            a, ref = (v[k][:n].view(np.float64).reshape(-1, NO) for v in (new, exact))
            for c in range(NO):
                limit = bar[c] * (length if k == 4 else 1.0)
                e_new = np.abs(a[:, c] - ref[:, c])
                worst = int(np.argmax(e_new - limit))
                lim = float(limit[worst]) if k == 4 else float(limit)
                print("fast %s %s form, %s of %s: e_new %.3e  e_old %.3e  bar %.3e  (e_new / bar %.3f)"
                      % (name, form, side, names[c], e_new[worst], e_old[c], lim, e_new[worst] / lim if lim > 0 else 0.0))
                if not np.all(e_new <= limit):
                    failures.append((form, side, names[c], float(e_new[worst]), float(e_old[c]), lim))
    ctx.close()
    assert not failures, failures


def test_fast_flavour_goddard():
    ctx, problem, z3 = goddard_m3("fast", step_nbr=20)
    fast_flavour_check("goddard", ctx, perturbed(z3, 22, rel=0.002), "goddard")


def test_fast_flavour_vtol():
    ctx, table, zstar = vtol_path4("fast")
    Z = np.concatenate([zstar[None, :], perturbed(zstar, 5, rel=0.01, seed=13)])
    fast_flavour_check("vtolUAV", ctx, Z, "vtol", table=table, unfused=(2,))


# ---- the sweep tool -----------------------------------------------------------------------------------------------------------------

def test_sweep_tool_writes_the_observe_file_and_record(tmp_path):
    out = str(tmp_path / "obs")
    run = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--starts", "64", "--rk4-steps", "50", "--observe-out", out], cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    entry = rec["observe"]
    names = ["r", "v", "norm_u", "drag", "drag_acc", "fuel_rate"]
    assert {"rows", "nbad_rows"} | set(names) <= set(entry)
    npz = np.load(entry["file"])
    assert entry["file"] == out + ".rank0.npz"
    assert sorted(npz.files) == sorted(["index", "names", "ymin", "ymax", "tmin", "tmax", "integral", "count", "nbad"])
    assert npz["names"].tolist() == names
    k = entry["rows"]
    assert k == rec["converged"] == len(npz["index"]) > 0
    assert npz["ymin"].shape == (k, 1, 6) == npz["integral"].shape and np.all(npz["count"] == 51) and npz["nbad"].shape == (k, 1)
    assert entry["nbad_rows"] == int(np.sum(npz["nbad"].sum(axis=1) > 0)) == 0
    for c, name in enumerate(names):
        total = npz["integral"][:, 0, c]
        assert entry[name] == {"min": float(npz["ymin"][:, :, c].min()), "max": float(npz["ymax"][:, :, c].max()),
                               "integral_median": float(np.median(total))}, name
    print("sweep of 64 starts, N = 50: %d converged; peak drag %.4e, burnt fuel (median) %.6f, peak r %.6f"
          % (k, entry["drag"]["max"], entry["fuel_rate"]["integral_median"], entry["r"]["max"]))
    assert np.all(npz["ymin"] <= npz["ymax"]) and np.all(npz["tmin"] >= 0.0) and entry["fuel_rate"]["integral_median"] > 0.0
    bad = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--model", "interceptor", "--observe-out", out], cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--observe-out" in bad.stderr
