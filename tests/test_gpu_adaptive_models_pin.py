"""GPU: the interceptor (InterceptorT::compute_traj<1>: the chart-change hook before every step, two phases, the hand-back) and
vtolUAV (with its obstacle map) under the adaptive Dormand-Prince integrator, BOTH flavours, pinned to a 240-bit replay decision by
decision (tests/adaptive_models_reference.py; the fixture tests/golden/adaptive_models_pin.npz is written by
tests/golden/make_adaptive_models_golden.py and checked on the CPU by tests/test_adaptive_models_pin_cpu.py).

Every comparison is |got - value| <= bound with factor 1; the bounds are derived (running error analysis of the replayed loop with
the models' own budgets) and lie many orders below one step's local error, which is the size of a stale FSAL derivative, a hook that
is not called before every step, a first step formed from the wrong start time, a stage that is not switched or a missing hand-back.
The ratios these tests print are observations (profiles/adaptive_models_pin_gpu_tests.txt), none of them is a tolerance.  The fixture
holds decidable scenarios only, and no test leaves one out."""
import os

import numpy as np
import pytest

import interceptor_reference as ir
import vtol_reference as vr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "adaptive_models_pin.npz"))
PREFIX = {"interceptor": "i_", "vtol": "v_"}
CASES = [("interceptor", "ref"), ("interceptor", "fast"), ("vtol", "ref"), ("vtol", "fast")]
IDS = ["%s-%s" % c for c in CASES]
U = 2.0 ** -53


def _context(model, fl):
    from socp_amd import capi
    c = capi.Context(capi.MODEL_INTERCEPTOR if model == "interceptor" else capi.MODEL_VTOLUAV)
    c.set_variant(capi.VARIANT_LANE_EXACT if fl == "ref" else capi.VARIANT_LANE_FAST)
    return c


def _configure(c, model, i):
    from socp_amd import capi
    p = PREFIX[model]
    if model == "vtol":
        c.set_map(FIX["table_" + str(FIX["map_names"][FIX["v_map"][i]])])
    c.set_params(FIX[p + "P"][i])
    c.set_step_number(int(FIX[p + "step_nbr"][i]))
    c.set_integrator(capi.INT_DOPRI5, float(FIX[p + "tol"][i]))


def ratios(got, val, B):
    err = np.abs(got - val)
    with np.errstate(all="ignore"):
        return np.where(err == 0, 0.0, np.where(np.isnan(err), np.inf, err / B))


def _check(what, model, fl, i, got, val, B):
    """|got - val| <= B, factor 1; a failure names the scenario, the door, the row and component, error / bound and the trail."""
    got = np.asarray(got)
    assert got.shape == np.shape(val), "%s: %s %s scenario %d has shape %s, the fixture %s; trail %s" % (
        what, model, fl, i, got.shape, np.shape(val), str(FIX[PREFIX[model] + "trail"][i]))
    r = ratios(got, val, B)
    if not np.all(r <= 1.0):
        k = tuple(int(v) for v in np.unravel_index(np.argmax(r), r.shape))
        pytest.fail("%s: %s %s scenario %d (row, component) %s: error / bound = %.3g; trail %s"
                    % (what, model, fl, i, k, r[k], str(FIX[PREFIX[model] + "trail"][i])))
    return float(r.max())


_doors = {}


def doors(model, fl):
    """Every scenario of a model through every entry point that integrates adaptively and hands out a state, once per flavour:
    [dict(batch, res, dense = (times, rows, aux or None), trace = (times, rows, aux), extrema, observe)]."""
    if (model, fl) in _doors:
        return _doors[(model, fl)]
    p = PREFIX[model]
    c = _context(model, fl)
    D, S = c.dim, c.s
    W = c.trace_width()
    out = []
    try:
        for i in range(len(FIX[p + "tf"])):
            _configure(c, model, i)
            X0, t0, tf = FIX[p + "X0"][i], float(FIX[p + "t0"][i]), float(FIX[p + "tf"][i])
            d = {"batch": c.integrate_batch(t0, tf, X0[None, :])[0]}
            # a one-segment problem whose final rows return the end state: all FIXED against zeros gives X[j], all FREE gives X[j + D]
            # (vtolUAV's FREE row also carries weights times X[j] - xd[j]: there xd is the fixture's end state, see residual_reference)
            res = np.empty(S)
            for mode, half in ((0, slice(0, D)), (1, slice(D, S))):
                mx = np.zeros((2, D), dtype=np.int32)
                mx[1] = mode
                xnode = np.zeros((2, S))
                if model == "vtol" and mode == 1:
                    xnode[1, :D] = FIX[p + "states"][i][FIX[p + "nrows"][i] - 1][:D]
                c.problem_set([0, 0], mx, np.array([t0, tf]), xnode)
                res[half] = c.residual(X0)[D:2 * D]
            d["res"] = res
            # (the problem in force is now the all-FREE one: trace, extrema and observe integrate its one segment from X0)
            if model == "interceptor":
                d["dense"] = c.integrate_dense_aux(t0, tf, X0, cap=64)
            else:
                d["dense"] = c.integrate_dense(t0, tf, X0, cap=64) + (None,)
            rows, count = c.trace_batch(X0[None, :], stride=1)
            k = int(count[0, 0])
            d["trace"] = (rows[0, 0, :k, 0].copy(), rows[0, 0, :k, 1:1 + S].copy(), rows[0, 0, :k, W - 2:].copy())
            d["extrema"] = int(c.extrema_batch(X0[None, :], what=0)["count"][0, 0])
            d["observe"] = int(c.observe_batch(X0[None, :])["count"][0, 0]) if c.has_observe() else None
            out.append(d)
    finally:
        c.close()
    _doors[(model, fl)] = out
    return out


def residual_reference(model, i, val, B):
    """What the final rows make of the end state, with every rounding they add counted.  The interceptor's final_row divides the
    altitude row by HR and adds muV to the free-velocity row: fl(x / HR) of a device x within B of val differs from the double
    fl(val / HR) by at most B / HR + u |x / HR| + u |val / HR|, and likewise for the sum."""
    val, B = val.copy(), B.copy()
    if model == "interceptor":
        P = FIX["i_P"][i]
        hr, muv = P[ir.HR], P[ir.MUV]
        val[0], B[0] = val[0] / hr, (B[0] / hr + 2 * U * (abs(val[0]) + B[0]) / hr) * (1 + 2.0 ** -50)
        val[7], B[7] = val[7] + muv, (B[7] + 2 * U * (abs(val[7] + muv) + B[7])) * (1 + 2.0 ** -50)
    else:
        # vtolUAV's FREE row is X[j + D] - w dx - 0.02 dx with dx = X[j] - xd[j] and w = invSigma (nWP_tot - nWP).  With xd[j] the
        # fixture's value, dx is the device's own deviation, |dx| <= B[j] (the subtraction of two doubles that close is exact):
        # the row is within B[j + D] + (|w| + 0.02) B[j] of val[j + D], plus one rounding of each of the two subtractions; the
        # roundings of w and of the two small products are relative to terms of the size of B[j] and go into the last factor
        P = FIX["v_P"][i]
        w = abs(P[vr.I_INVSIGMA] * (P[vr.I_NWP_TOT] - P[vr.I_NWP])) + 0.02
        small = w * B[:6]
        B[6:] = (B[6:] + small + 2 * U * (np.abs(val[6:]) + B[6:] + small)) * (1 + 2.0 ** -40)
    return val, B


@pytest.mark.parametrize("model,fl", CASES, ids=IDS)
def test_end_state_through_every_door(model, fl, capsys):
    """integrate_batch (traj_lane_kernel), the residual (segment_residual), integrate_dense[_aux] and trace_batch(stride = 1): the
    fixture's end state -- for the interceptor handed back in chart 1 -- within its bound through each; in the reference-order flavour
    the doors are bit-equal among themselves where they report the same quantity."""
    p = PREFIX[model]
    top = {}
    for i, d in enumerate(doors(model, fl)):
        r = FIX[p + "nrows"][i] - 1
        val, B = FIX[p + "states"][i][r], FIX[p + "B_" + fl][i][r]
        ends = {"batch": d["batch"], "dense": d["dense"][1][-1], "trace": d["trace"][1][-1]}
        for door, got in ends.items():
            top[door] = max(top.get(door, 0.0), _check(door, model, fl, i, got, val, B))
        rv, rB = residual_reference(model, i, val, B)
        top["residual"] = max(top.get("residual", 0.0), _check("residual", model, fl, i, d["res"], rv, rB))
        if fl == "ref":
            for door, got in ends.items():
                assert np.array_equal(got, ends["batch"]), (door, i)
            same = (rv == val) & (rB == B)                        # the rows final_row hands through untouched
            assert np.array_equal(d["res"][same], d["batch"][same]), ("residual", i)
    with capsys.disabled():
        print("\n%s %s end state, largest err/bound: %s" % (model, fl, " ".join("%s %.3f" % kv for kv in top.items())))


@pytest.mark.parametrize("model,fl", CASES, ids=IDS)
def test_rows_of_dense_and_trace(model, fl, capsys):
    """The rows of integrate_dense[_aux] and trace_batch: exactly the fixture's number of rows (for the interceptor: per phase, plus the
    extra final row), its accepted times and the raw-chart states at them, each within its own bound; the interceptor's stage and
    chart columns equal to the fixture's, exactly; the count of extrema_batch (and of observe_batch where the model has one) equal to
    the row count."""
    p = PREFIX[model]
    top = {}
    for i, d in enumerate(doors(model, fl)):
        n = int(FIX[p + "nrows"][i])
        trail = str(FIX[p + "trail"][i])
        for door in ("dense", "trace"):
            times, rows, aux = d[door]
            assert len(times) == n, "%s: %s %s scenario %d has %d rows, the fixture %d; trail %s" % (door, model, fl, i, len(times), n, trail)
            top[door + " t"] = max(top.get(door + " t", 0.0),
                                   _check(door + " times", model, fl, i, times, FIX[p + "times"][i][:n], FIX[p + "Bt_" + fl][i][:n]))
            top[door + " X"] = max(top.get(door + " X", 0.0),
                                   _check(door + " rows", model, fl, i, rows, FIX[p + "states"][i][:n], FIX[p + "B_" + fl][i][:n]))
            if model == "interceptor":
                assert np.array_equal(aux[:, 0], FIX["i_stage"][i][:n]), "%s: stage column, scenario %d: %s; trail %s" % (door, i, aux[:, 0], trail)
                assert np.array_equal(aux[:, 1], FIX["i_chart"][i][:n]), "%s: chart column, scenario %d: %s; trail %s" % (door, i, aux[:, 1], trail)
                # the phases: a row whose time does not advance starts the second phase, the last repeats tf
                n1 = int(FIX["i_phase_rows"][i][0])
                assert times[n - 1] == FIX["i_tf"][i] and times[0] == FIX["i_t0"][i]
                if FIX["i_phase_rows"][i][1] > 0:
                    assert times[n1] == times[n1 - 1] == FIX["i_P"][i][ir.PROP] / FIX["i_P"][i][ir.Q] and aux[n1, 0] == 0.0 and aux[n1 - 1, 0] == 1.0
        if fl == "ref":
            assert all(np.array_equal(a, b) for a, b in zip(d["dense"][:2], d["trace"][:2])), i
        assert d["extrema"] == n, ("extrema_batch count", i, d["extrema"], n, trail)
        assert d["observe"] is None or d["observe"] == n, ("observe_batch count", i, d["observe"], n, trail)
    with capsys.disabled():
        print("\n%s %s rows, largest err/bound: %s" % (model, fl, " ".join("%s %.3f" % kv for kv in top.items())))


def _interceptor_rows():
    """70 interceptor starts of one parameter block with t1 = 1/16, for one wavefront and a bit: flight-path angles that cross the
    chart limit at different steps (1.42 .. 1.47), start beyond it (1.5, 1.55) or never get there (0.3, 0.9); segments that end
    before t1 (one phase), start after it (one phase, coasting) or straddle it (two phases)."""
    i = int(np.flatnonzero(FIX["i_phase_rows"][:, 1] > 0)[0])
    P = FIX["i_P"][i]
    gammas = [1.46, 1.5, 0.3, 1.42, 1.44, 1.47, 1.55, 0.9, 1.45, 1.465]
    spans = [(0.0, 0.125), (0.0, 0.0625), (0.03125, 0.25), (0.0, 0.03125), (0.125, 0.25), (0.0, 0.25), (0.03125, 0.0625)]
    X0 = np.repeat(FIX["i_X0"][i][None, :], 70, axis=0)
    X0[:, 2] = [gammas[b % len(gammas)] for b in range(70)]
    t0 = np.array([spans[b % len(spans)][0] for b in range(70)])
    tf = np.array([spans[b % len(spans)][1] for b in range(70)])
    return P, X0, t0, tf


def _vtol_rows():
    """70 vtolUAV starts under one scenario's parameter block and map: the fixture's starts over a spread of final times, so that
    neighbouring lanes take different numbers of trial steps."""
    i = int(np.argmax(FIX["v_ntrials"]))
    X0 = np.stack([FIX["v_X0"][b % len(FIX["v_X0"])] for b in range(70)])
    tf = np.linspace(0.004, 0.25, 70)[np.random.default_rng(5).permutation(70)]
    return i, X0, np.zeros(70), tf


@pytest.mark.parametrize("model,fl", CASES, ids=IDS)
def test_rows_do_not_depend_on_the_batch(model, fl):
    """Per-lane step control, per-lane chart and stage under the exec mask: each of 70 rows of one batch is bit-equal to the same row
    integrated alone.  Then row 5 gets a NaN in its start: it comes back all-NaN (500 rejected tries, the poison path) and the other
    69 are still bit-equal to their solo runs.  A NaN start is an input the integrator has an answer for, not a fault."""
    from socp_amd import capi
    c = _context(model, fl)
    try:
        if model == "interceptor":
            P, X0, t0, tf = _interceptor_rows()
            c.set_params(P)
            c.set_step_number(2)
            c.set_integrator(capi.INT_DOPRI5, 1e-7)
        else:
            i, X0, t0, tf = _vtol_rows()
            _configure(c, "vtol", i)
        assert len(X0) == 70
        whole = c.integrate_batch(t0, tf, X0)
        solo = np.stack([c.integrate_batch(t0[b:b + 1], tf[b:b + 1], X0[b:b + 1])[0] for b in range(70)])
        assert np.all(np.isfinite(whole))
        assert np.array_equal(whole, solo)
        # the lanes of the first wavefront really differ in what they do
        counts = {len(c.integrate_dense(t0[b], tf[b], X0[b], cap=64)[0]) for b in range(0, 14)}
        assert len(counts) >= 3, counts
        bad = X0.copy()
        bad[5, 3] = np.nan
        got = c.integrate_batch(t0, tf, bad)
        assert np.all(np.isnan(got[5]))
        keep = np.arange(70) != 5
        assert np.array_equal(got[keep], solo[keep])
    finally:
        c.close()


def test_report_share_of_the_pow_budget(capsys):
    """Not a check of the device: what the fixture says about C_POW = 16 (dopri5_reference.py).  Its largest share of any end-state
    bound stays below one percent."""
    with capsys.disabled():
        print()
        for model, p in PREFIX.items():
            for fl in ("ref", "fast"):
                share = float(FIX[p + "pow_" + fl].max())
                print("%s %s: largest share of C_POW in an end-state bound %.3g" % (model, fl, share))
                assert share < 0.01
