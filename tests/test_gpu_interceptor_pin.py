"""GPU: the interceptor (socp_amd/csrc/models_interceptor.hpp) in BOTH flavours pinned to a 240-bit evaluation: right-hand side, control
and Hamiltonian row by row and component by component within a derived bound, both directions of the chart change, the batch round
trip, and four short segments (tests/interceptor_reference.py; the fixture tests/golden/interceptor_pin.npz is written by
tests/golden/make_interceptor_pin_golden.py and checked on the CPU by tests/test_interceptor_pin_cpu.py).

The bounds are derived (running error analysis; rcp / rsqrt 2u, exp_glibc 2u, the short sincos 8u + 2^-108 |k|; the device library's
sin, cos, acos 8u, tan 10u, atan2 12u, exp 6u -- the OpenCL full-profile limits, a specification and not a measurement); the ratios
these tests print are observations (profiles/interceptor_pin_gpu_tests.txt) and none of them is a tolerance.  The chart change is
shared text, compiled with contraction in the throughput translation unit: both flavours are held to the reference-order bound.

The 2 -> 1 direction is judged on the DEVICE's own chart-2 row taken as exact doubles, so its 240-bit value is formed here (mpmath);
everything else reads the fixture only."""
import os

import numpy as np
import pytest

import fast_reference as fr
import interceptor_reference as ir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "interceptor_pin.npz"))
GROUPS = [str(g) for g in FIX["group_names"]]
CC_GROUPS = [str(g) for g in FIX["cc_group_names"]]
N, NCC = len(FIX["X"]), len(FIX["cc_X"])
U = 2.0 ** -53
FLAVOURS = ["fast", "reference-order"]


@pytest.fixture(scope="module")
def ctx():
    from socp_amd import capi
    c = capi.Context(capi.MODEL_INTERCEPTOR)
    yield c
    c.close()


def _variant(flavour):
    from socp_amd import capi
    return capi.VARIANT_LANE_FAST if flavour == "fast" else capi.VARIANT_LANE_EXACT


def batch(ctx, flavour, rows):
    """(rhs[., 12], control[., 2], H[.]) of the fixture rows `rows`: one eval_batch of each kind per parameter block, every row with
    its own time and its own (stage, chart) pair."""
    from socp_amd import capi
    rows = np.asarray(rows)
    rhs, ctl, ham = np.full((len(rows), 12), np.nan), np.full((len(rows), 2), np.nan), np.full(len(rows), np.nan)
    ctx.set_variant(_variant(flavour))
    try:
        for b in sorted(set(FIX["block"][rows])):
            at = np.flatnonzero(FIX["block"][rows] == b)
            sel = rows[at]
            sw = np.stack([FIX["stage"][sel], FIX["chart"][sel]], axis=1).astype(np.float64)
            ctx.set_params(FIX["blocks"][b])
            rhs[at] = ctx.eval_batch(capi.EVAL_RHS, FIX["t"][sel], FIX["X"][sel], sw=sw)
            ctl[at] = ctx.eval_batch(capi.EVAL_CONTROL, FIX["t"][sel], FIX["X"][sel], sw=sw)[:, :2]
            ham[at] = ctx.eval_batch(capi.EVAL_HAMILTONIAN, FIX["t"][sel], FIX["X"][sel], sw=sw)[:, 0]
    finally:
        ctx.set_variant(capi.VARIANT_AUTO)
    return rhs, ctl, ham


_cache = {}


def evaluate(ctx, flavour):
    if flavour not in _cache:
        out = batch(ctx, flavour, np.arange(N))
        for a in out:
            a.setflags(write=False)
        _cache[flavour] = out
    return _cache[flavour]


def ratios(got, val, B):
    """|got - val| / B per component; 0 where they are equal (a bound of zero demands equality)."""
    with np.errstate(all="ignore"):
        err = np.abs(got - val)
        return np.where(got == val, 0.0, np.where(np.isnan(err), np.inf, err / B))


def report(title, group, names, r):
    for g in sorted(set(group)):
        print("%s %-14s max err/B per component: %s" % (title, names[g], " ".join("%.3f" % v for v in np.atleast_2d(r[group == g]).max(axis=0))))


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_rhs_within_bound(ctx, flavour, capsys):
    """Decidable rows of every group: |rhs - value| <= B per component (B_fast / B_ref); finite on every row, the costates of 1e-170
    and 1e160 included (the 240-bit value of every fixture row is finite)."""
    bound = "Bfast" if flavour == "fast" else "Bref"
    rhs = evaluate(ctx, flavour)[0]
    dec = FIX["dec"]
    r = ratios(rhs, FIX["val"], FIX[bound])
    with capsys.disabled():
        print()
        report("%s rhs/%s" % (flavour, bound), FIX["group"][dec], GROUPS, r[dec])
    assert np.all(np.isfinite(rhs))
    assert np.all(r[dec] <= 1.0), np.argwhere(r[dec] > 1.0)[:8]


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_undecidable_rows_lie_on_an_adjacent_branch(ctx, flavour):
    bound = "Bfast" if flavour == "fast" else "Bref"
    und = FIX["und"]
    assert len(und)
    rhs, ctl, ham = evaluate(ctx, flavour)
    for got, key, b in ((rhs[und], "val", bound), (ctl[und], "u", "Bu"), (ham[und], "H", "BH")):
        here = ratios(got, FIX[key][und], FIX[b][und])
        there = ratios(got, FIX["alt_" + key], FIX["alt_" + b])
        assert np.all(np.minimum(here, there) <= 1.0), (key, np.argwhere(np.minimum(here, there) > 1.0))


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_control_and_hamiltonian_within_bound(ctx, flavour, capsys):
    """Both flavours evaluate the control and the Hamiltonian by the reference-order text (the throughput flavour under contraction:
    fewer roundings than the bound counts)."""
    _, u, h = evaluate(ctx, flavour)
    dec = FIX["dec"]
    ru, rh = ratios(u, FIX["u"], FIX["Bu"]), ratios(h, FIX["H"], FIX["BH"])
    with capsys.disabled():
        print()
        report("%s control/B_u" % flavour, FIX["group"][dec], GROUPS, ru[dec])
        report("%s hamiltonian/B_H" % flavour, FIX["group"][dec], GROUPS, rh[dec][:, None])
    assert np.all(np.isfinite(u)) and np.all(np.isfinite(h))
    assert np.all(ru[dec] <= 1.0), np.argwhere(ru[dec] > 1.0)[:8]
    assert np.all(rh[dec] <= 1.0), np.flatnonzero(rh[dec] > 1.0)[:8]


@pytest.mark.parametrize("B", [1, 63, 64, 65])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_rows_do_not_depend_on_the_batch(ctx, flavour, B):
    """The first B rows of the shipped block, alone, are bit-equal to the same rows of the whole batch: below, at and past one 64-lane
    wave, rows of both charts and both stages side by side."""
    rows = np.flatnonzero(FIX["block"] == 0)
    assert len(rows) > 130 and len({(c, s) for c, s in zip(FIX["chart"][rows[:65]], FIX["stage"][rows[:65]])}) == 4
    whole = evaluate(ctx, flavour)
    part = batch(ctx, flavour, rows[:B])
    for p, w in zip(part, whole):
        assert len(p) == B and np.array_equal(p, w[rows[:B]])


def chart21_ratio(P, X2, got):
    """|got - value| / B of the 240-bit ConversionState21 of the doubles X2; on an undecidable row the smaller of the two branches."""
    e = ir.evaluate_chart(P, False, X2)
    r = ratios(got, e["value"], e["B"])
    if not e["decidable"]:
        alt = ir.evaluate_chart(P, False, X2, flip=e["undecided"])
        r = np.minimum(r, ratios(got, alt["value"], alt["B"]))
    return r, bool(np.all(e["B"] <= 1e-10 * np.maximum(1.0, np.abs(e["value"]))))


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_chart_change_both_directions_and_round_trip(ctx, flavour, capsys):
    """chartLimit = 2 makes every state change chart, one step of zero length adds nothing: the dense rows of integrate_dense_aux(t0, t0,
    X) are the start, the state after set_chart (chart 2) and the handed-back state (chart 1).  1 -> 2 against the 240-bit
    ConversionState12 of the input (on the pivot-tie rows, l == L, against the smaller of the two elimination orders' ratios, as an
    undecidable row is judged everywhere); 2 -> 1 against the 240-bit ConversionState21 of the device's own chart-2 row; the batch round trip
    returns the dense call's last row bit for bit.  The planar group (chi = 0, pi: acos(sqrt(1 - cos^2 gamma sin^2 chi)) keeps half the
    digits in the reference's own formula) is held to its large bound and reported, not counted as informative."""
    assert fr.HAVE_MPMATH, "this test forms the 240-bit value of the device's own chart-2 row: it needs mpmath"
    from socp_amd import capi
    P = FIX["blocks"][int(FIX["cc_block"])]
    X = FIX["cc_X"]
    ctx.set_params(P)
    ctx.set_step_number(1)
    ctx.set_variant(_variant(flavour))
    try:
        rows = [ctx.integrate_dense_aux(0.0, 0.0, x, cap=8) for x in X]
        back = ctx.integrate_batch(0.0, 0.0, X)
    finally:
        ctx.set_variant(capi.VARIANT_AUTO)
        ctx.set_step_number(50)
    for (t, d, aux), x in zip(rows, X):
        assert len(t) == 3 and np.all(t == 0.0) and np.array_equal(d[0], x)
        assert tuple(aux[0]) == (1.0, 1.0) and tuple(aux[1]) == (1.0, 2.0)
    X2 = np.array([d[1] for _, d, _ in rows])
    X1 = np.array([d[2] for _, d, _ in rows])
    assert np.all(np.isfinite(X2)) and np.all(np.isfinite(X1))
    assert np.array_equal(back, X1)
    r12 = ratios(X2, FIX["cc_val12"], FIX["cc_B12"])
    und12 = FIX["cc_und12"]                             # pivot ties (l == L): either elimination order, each with its own bound
    r12[und12] = np.minimum(r12[und12], ratios(X2[und12], FIX["alt_cc_val12"], FIX["alt_cc_B12"]))
    both = [chart21_ratio(P, x2, x1) for x2, x1 in zip(X2, X1)]
    r21 = np.array([b[0] for b in both])
    inf21 = np.array([b[1] for b in both])
    out = FIX["cc_group"] != CC_GROUPS.index("planar")
    with capsys.disabled():
        print()
        report("%s chart change 1->2 / B" % flavour, FIX["cc_group"], CC_GROUPS, r12)
        report("%s chart change 2->1 / B" % flavour, FIX["cc_group"], CC_GROUPS, r21)
        print("%s chart change 2->1: informative rows outside the planar group %d of %d" % (flavour, inf21[out].sum(), out.sum()))
    assert len(und12) and all("pivot" in str(n) for n in FIX["cc_und12_names"])
    assert np.all(r12 <= 1.0), np.argwhere(r12 > 1.0)[:8]
    assert np.all(r21 <= 1.0), np.argwhere(r21 > 1.0)[:8]
    assert inf21[out].mean() >= 0.9


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_short_segments_against_mpf_rk4(ctx, flavour, capsys):
    """Five steps per stage from four starts -- powered only, across t1, a start beyond the chart limit, one that crosses the limit
    mid-way and is handed back -- against the same recurrence in mpf with the chart decisions on exact values.  The yardstick is the
    pinned reference-order CPU oracle's own deviation from the mpf trajectory (per component, the largest of the four): either flavour
    stays within 8x that figure plus 8 u |X|."""
    from socp_amd import capi
    ctx.set_params(FIX["blocks"][0])
    ctx.set_step_number(int(FIX["seg_N"]))
    ctx.set_variant(_variant(flavour))
    try:
        Xf = ctx.integrate_batch(FIX["seg_t0"], FIX["seg_tf"], FIX["seg_X0"])
    finally:
        ctx.set_variant(capi.VARIANT_AUTO)
        ctx.set_step_number(50)
    ref, dev = FIX["seg_mpf"], FIX["seg_dev"]
    err = np.abs(Xf - ref)
    allowed = 8 * dev[None, :] + 8 * U * np.abs(ref)
    with capsys.disabled(), np.errstate(all="ignore"):
        print()
        print("segments: oracle deviation per component:      %s" % " ".join("%.2e" % v for v in dev))
        print("segments: %s deviation per component: %s" % (flavour, " ".join("%.2e" % v for v in err.max(axis=0))))
        print("segments: %s err/allowed per component: %s" % (flavour, " ".join("%.3f" % v for v in (err / allowed).max(axis=0))))
    assert np.all(np.isfinite(Xf))
    assert np.all(err <= allowed), np.argwhere(err > allowed)[:8]
