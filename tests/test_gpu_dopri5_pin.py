"""GPU: the adaptive Dormand-Prince integrator (Lane::dopri5_try / integrate_dopri5, socp_amd/csrc/integrator.hpp, and its copy in
traj_var_wave_dopri5_kernel, variational.hpp) pinned to a 240-bit replay of the whole controller loop on short segments
(tests/dopri5_reference.py; the fixture tests/golden/dopri5_pin.npz is written by tests/golden/make_dopri5_golden.py and checked on
the CPU by tests/test_dopri5_pin_cpu.py).

Every comparison is |got - value| <= bound with factor 1; the bounds are derived (running error analysis of the replayed loop) and
sit many orders below what any change of the tableau, the error norm or the controller does to a step size.  The ratios these
tests print are observations (profiles/dopri5_pin_gpu_tests.txt), none of them is a tolerance.  The fixture holds decidable
scenarios only, and no test leaves one out."""
import os

import numpy as np
import pytest

from conftest import goddard_costate_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "dopri5_pin.npz"))
PREFIX = {"goddard": "g_", "covid": "c_", "dint": "d_", "dint_aug": "a_"}
CASES = [("goddard", "ref"), ("goddard", "fast"), ("covid", "ref"), ("covid", "fast"), ("dint", "ref")]
IDS = ["%s-%s" % c for c in CASES]


def _context(model, fl):
    from socp_amd import capi
    c = capi.Context({"goddard": capi.MODEL_GODDARD, "covid": capi.MODEL_COVID19, "dint": capi.MODEL_DOUBLE_INTEGRATOR,
                      "dint_aug": capi.MODEL_DOUBLE_INTEGRATOR}[model])
    if model in ("goddard", "covid"):
        c.set_variant(capi.VARIANT_LANE_EXACT if fl == "ref" else capi.VARIANT_LANE_FAST)
    return c


def _configure(c, model, i):
    from socp_amd import capi
    p = PREFIX[model]
    c.set_params(FIX[p + "P"][i])
    c.set_step_number(int(FIX[p + "step_nbr"][i]))
    c.set_integrator(capi.INT_DOPRI5, float(FIX[p + "tol"][i]))
    c.set_switching_times(FIX[p + "sw"][i])


def ratios(got, val, B):
    err = np.abs(got - val)
    with np.errstate(all="ignore"):
        return np.where(err == 0, 0.0, np.where(np.isnan(err), np.inf, err / B))


def _check(what, model, fl, i, got, val, B):
    """|got - val| <= B, factor 1; a failure names the scenario, the component, error / bound and the fixture's decision trail."""
    r = ratios(got, val, B)
    if not np.all(r <= 1.0):
        k = tuple(int(v) for v in np.unravel_index(np.argmax(r), r.shape))
        pytest.fail("%s: %s %s scenario %d component %s: error / bound = %.3g; trail %s"
                    % (what, model, fl, i, k, r[k], str(FIX[PREFIX[model] + "trail"][i])))
    return float(r.max())


_doors = {}


def doors(model, fl):
    """Every scenario of a model through the four doors, once per flavour: [dict(batch, res, dense = (times, rows), trace = ...)]."""
    if (model, fl) in _doors:
        return _doors[(model, fl)]
    p = PREFIX[model]
    c = _context(model, fl)
    D, S = c.dim, c.s
    out = []
    try:
        for i in range(len(FIX[p + "tf"])):
            _configure(c, model, i)
            X0, tf = FIX[p + "X0"][i], float(FIX[p + "tf"][i])
            d = {"batch": c.integrate_batch(0.0, tf, X0[None, :])[0]}
            # a one-segment problem whose final rows are the end state: all FIXED against zeros gives X[j], all FREE gives X[j + D]
            res = np.empty(S)
            for mode, half in ((0, slice(0, D)), (1, slice(D, S))):
                mx = np.zeros((2, D), dtype=np.int32)
                mx[1] = mode
                c.problem_set([0, 0], mx, np.array([0.0, tf]), np.zeros((2, S)))
                res[half] = c.residual(X0)[D:2 * D]
            d["res"] = res
            d["dense"] = c.integrate_dense(0.0, tf, X0)
            rows, count = c.trace_batch(X0[None, :], stride=1)
            k = int(count[0, 0])
            d["trace"] = (rows[0, 0, :k, 0].copy(), rows[0, 0, :k, 1:1 + S].copy())
            out.append(d)
    finally:
        c.close()
    _doors[(model, fl)] = out
    return out


@pytest.mark.parametrize("model,fl", CASES, ids=IDS)
def test_end_state_through_four_doors(model, fl, capsys):
    """integrate_batch (traj_lane_kernel), residual (segment_residual), integrate_dense and trace_batch(stride = 1): the fixture's end
    state within its bound through each; in the reference-order flavour the four are bit-equal among themselves."""
    p = PREFIX[model]
    top = {}
    for i, d in enumerate(doors(model, fl)):
        r = FIX[p + "nrows"][i] - 1
        val, B = FIX[p + "states"][i][r], FIX[p + "B_" + fl][i][r]
        ends = {"batch": d["batch"], "residual": d["res"], "dense": d["dense"][1][-1], "trace": d["trace"][1][-1]}
        for door, got in ends.items():
            top[door] = max(top.get(door, 0.0), _check(door, model, fl, i, got, val, B))
        if fl == "ref":
            for door, got in ends.items():
                assert np.array_equal(got, ends["batch"]), (door, i)
    with capsys.disabled():
        print("\n%s %s end state, largest err/bound: %s" % (model, fl, " ".join("%s %.3f" % kv for kv in top.items())))


@pytest.mark.parametrize("model,fl", CASES, ids=IDS)
def test_accepted_steps_of_dense_and_trace(model, fl, capsys):
    """The rows of integrate_dense and trace_batch: exactly the fixture's number of rows, its accepted times and the states at
    them, each within its own bound."""
    p = PREFIX[model]
    top = 0.0
    for i, d in enumerate(doors(model, fl)):
        n = int(FIX[p + "nrows"][i])
        for door in ("dense", "trace"):
            times, rows = d[door]
            assert len(times) == n, "%s: %s %s scenario %d has %d rows, the fixture %d; trail %s" % (
                door, model, fl, i, len(times), n, str(FIX[p + "trail"][i]))
            top = max(top, _check(door + " times", model, fl, i, times, FIX[p + "times"][i][:n], FIX[p + "Bt_" + fl][i][:n]))
            top = max(top, _check(door + " rows", model, fl, i, rows, FIX[p + "states"][i][:n], FIX[p + "B_" + fl][i][:n]))
    with capsys.disabled():
        print("\n%s %s accepted times and states, largest err/bound: %.3f" % (model, fl, top))


def _wave_order():
    """Augmented scenarios ordered so that neighbouring blocks take different numbers of trial steps (fewest, most, ...)."""
    by = list(np.argsort(FIX["a_ntrials"], kind="stable"))
    out = []
    while by:
        out.append(by.pop(0))
        if by:
            out.append(by.pop())
    return np.array(out)


def test_variational_wave_kernel_end_state(capsys):
    """integrate_batch(is_jac = 1) on the 156-element scenarios (traj_var_wave_dopri5_kernel: its own copy of the tableau and the
    controller, step control per wave).  Every scenario's (tol, step_nbr) runs ALL scenarios' starts as one batch, ordered so that
    neighbouring blocks take different numbers of trials; the row of the scenario itself is held to the fixture -- the scaled
    starts (sensitivity part x 1e6 and x 1e-6, which moves the norm's denominators across lanes and k slots) included.
    The kernel's per-problem-parameter path (pp_params) is reached only from inside the batched variational Jacobian, which hands
    out no end state: it is not pinned here."""
    order = _wave_order()
    nt = FIX["a_ntrials"][order]
    assert np.sum(nt[:-1] != nt[1:]) >= len(nt) // 2
    c = _context("dint_aug", "ref")
    top = 0.0
    try:
        for i in range(len(FIX["a_tf"])):
            _configure(c, "dint_aug", i)
            got = c.integrate_batch(0.0, FIX["a_tf"][order], FIX["a_X0"][order], is_jac=1)
            row = got[list(order).index(i)]
            r = FIX["a_nrows"][i] - 1
            top = max(top, _check("wave kernel", "dint_aug", "ref", i, row, FIX["a_states"][i][r], FIX["a_B_ref"][i][r]))
            assert np.all(np.isfinite(got))
    finally:
        c.close()
    assert set(FIX["a_group"]) == {0, 1, 2}
    with capsys.disabled():
        print("\nwave kernel end state, largest err/bound: %.3f" % top)


def _goddard_rows():
    """70 Goddard starts whose step counts differ: the fixture's smooth-law scenarios (their own start and tf) and
    goddard_costate_batch starts over a spread of tf."""
    sel = np.flatnonzero(np.all(FIX["g_P"] == FIX["g_P"][FIX["g_P"][:, 6] == 1.0][0], axis=1))
    X0 = [FIX["g_X0"][i] for i in sel]
    tf = [FIX["g_tf"][i] for i in sel]
    more = goddard_costate_batch(70 - len(sel), 1e-3)
    X0 += list(more)
    tf += list(np.linspace(0.004, 0.24, len(more)))
    return FIX["g_P"][sel[0]], FIX["g_sw"][sel[0]], np.array(X0), np.array(tf)


@pytest.mark.parametrize("fl", ["ref", "fast"])
def test_rows_do_not_depend_on_the_batch(fl):
    """Per-lane step control under the exec mask: each of 70 rows of one batch is bit-equal to the same row integrated alone.  Then
    row 5 gets a NaN in its start: it comes back all-NaN (500 rejected tries, the poison path) and its 63 wave neighbours are
    still bit-equal to their solo runs.  A NaN start is an input the integrator has an answer for, not a fault."""
    from socp_amd import capi
    P, sw, X0, tf = _goddard_rows()
    assert len(X0) == 70
    c = _context("goddard", fl)
    try:
        c.set_params(P)
        c.set_switching_times(sw)
        c.set_step_number(2)
        c.set_integrator(capi.INT_DOPRI5, 1e-5)
        whole = c.integrate_batch(0.0, tf, X0)
        solo = np.stack([c.integrate_batch(0.0, tf[b:b + 1], X0[b:b + 1])[0] for b in range(70)])
        assert np.all(np.isfinite(whole))
        assert np.array_equal(whole, solo)
        bad = X0.copy()
        bad[5, 3] = np.nan
        got = c.integrate_batch(0.0, tf, bad)
        assert np.all(np.isnan(got[5]))
        keep = np.arange(70) != 5
        assert np.array_equal(got[keep], solo[keep])
    finally:
        c.close()


def test_wave_kernel_blocks_do_not_depend_on_the_batch():
    """The same for the wave kernel: every block bit-equal to its solo run, and a NaN block among finite ones comes back all-NaN
    without touching its neighbours."""
    from socp_amd import capi
    order = _wave_order()
    X0, tf = FIX["a_X0"][order], FIX["a_tf"][order]
    c = _context("dint_aug", "ref")
    try:
        c.set_params(FIX["a_P"][0])
        c.set_step_number(2)
        c.set_integrator(capi.INT_DOPRI5, 1e-5)
        whole = c.integrate_batch(0.0, tf, X0, is_jac=1)
        solo = np.stack([c.integrate_batch(0.0, tf[b:b + 1], X0[b:b + 1], is_jac=1)[0] for b in range(len(X0))])
        assert np.all(np.isfinite(whole)) and np.array_equal(whole, solo)
        bad = X0.copy()
        bad[3, 40] = np.nan                                       # a sensitivity element: lane 40 of the block's wave
        got = c.integrate_batch(0.0, tf, bad, is_jac=1)
        assert np.all(np.isnan(got[3]))
        keep = np.arange(len(X0)) != 3
        assert np.array_equal(got[keep], solo[keep])
    finally:
        c.close()


def test_report_share_of_the_pow_budget(capsys):
    """Not a check of the device: what the fixture says about C_POW = 16 (OpenCL's limit for double pow; the device library's own
    figure is not known to us).  Its largest share of any end-state bound stays below one percent, so a pow that is worse than
    assumed by a factor of ten would still move no bound by more than a tenth."""
    with capsys.disabled():
        print()
        for model, p in PREFIX.items():
            for fl in ("ref", "fast"):
                if p + "pow_" + fl in FIX:
                    share = float(FIX[p + "pow_" + fl].max())
                    print("%s %s: largest share of C_POW in an end-state bound %.3g" % (model, fl, share))
                    assert share < 0.01
