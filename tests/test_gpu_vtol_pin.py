"""GPU: vtolUAV's right-hand side, control and Hamiltonian (socp_amd/csrc/models_vtol.hpp) in BOTH flavours pinned row by row and
component by component to a 240-bit evaluation, within a bound that carries each component's conditioning (tests/vtol_reference.py;
the fixture tests/golden/vtol_pin.npz is written by tests/golden/make_vtol_pin_golden.py and checked on the CPU by
tests/test_vtol_pin_cpu.py).  These tests read the fixture only.

Every evaluation goes through capi.Context.eval_batch, one set_map per map and one set_params per parameter block.  The bounds are
derived (running error analysis; rcp / rsqrt 2u each, the device library's tanh 10u and exp 6u -- the OpenCL full-profile limits, a
specification and not a measurement); the ratios these tests print are observations (profiles/vtol_pin_gpu_tests.txt) and none of
them is a tolerance."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "vtol_pin.npz"))
GROUPS = [str(g) for g in FIX["group_names"]]
MAPS = [str(m) for m in FIX["map_names"]]
N = len(FIX["X"])
U = 2.0 ** -53
PLAIN9 = [0, 1, 2, 6, 7, 8]             # within the stored rows 3-11: rows 3-5 and 9-11 (no map, no tanh)
MAPPED9 = [3, 4, 5]                     # rows 6-8
FLAVOURS = ["fast", "reference-order"]


@pytest.fixture(scope="module")
def ctx():
    from socp_amd import capi
    c = capi.Context(capi.MODEL_VTOLUAV)
    yield c
    c.close()


def _variant(flavour):
    from socp_amd import capi
    return capi.VARIANT_LANE_FAST if flavour == "fast" else capi.VARIANT_LANE_EXACT


_cache = {}


def evaluate(ctx, flavour, rows=None):
    """(rhs[., 12], control[., 3], H[.]) over the fixture's rows (all, or the index array `rows`): one eval_batch per map and
    parameter block; the whole fixture is cached per flavour."""
    from socp_amd import capi
    if rows is None and flavour in _cache:
        return _cache[flavour]
    idx = np.arange(N) if rows is None else np.asarray(rows)
    rhs, ctl, ham = np.full((N, 12), np.nan), np.full((N, 3), np.nan), np.full(N, np.nan)
    ctx.set_variant(_variant(flavour))
    try:
        for m in sorted(set(FIX["map"][idx])):
            ctx.set_map(FIX["table_" + MAPS[m]])
            on_map = idx[FIX["map"][idx] == m]
            for b in sorted(set(FIX["block"][on_map])):
                sel = on_map[FIX["block"][on_map] == b]
                ctx.set_params(FIX["blocks"][b])
                rhs[sel] = ctx.eval_batch(capi.EVAL_RHS, 0.0, FIX["X"][sel])
                ctl[sel] = ctx.eval_batch(capi.EVAL_CONTROL, 0.0, FIX["X"][sel])
                ham[sel] = ctx.eval_batch(capi.EVAL_HAMILTONIAN, 0.0, FIX["X"][sel])[:, 0]
    finally:
        ctx.set_variant(capi.VARIANT_AUTO)
    if rows is None:
        for a in (rhs, ctl, ham):
            a.setflags(write=False)
        _cache[flavour] = (rhs, ctl, ham)
        return _cache[flavour]
    return rhs[idx], ctl[idx], ham[idx]


def ratios(got, val, B):
    """|got - val| / B per component; 0 where they are equal (a bound of zero demands equality) or both NaN."""
    with np.errstate(all="ignore"):
        err = np.abs(got - val)
        same = (got == val) | (np.isnan(got) & np.isnan(val))
        return np.where(same, 0.0, np.where(np.isnan(err), np.inf, err / B))


def report(title, idx, r):
    for g in sorted(set(FIX["group"][idx])):
        sel = FIX["group"][idx] == g
        print("%s %-16s max err/B per component: %s" % (title, GROUPS[g], " ".join("%.3f" % v for v in np.atleast_2d(r[sel]).max(axis=0))))


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_rhs_within_bound(ctx, flavour, capsys):
    """Decidable rows of every group: |rhs - value| <= B per component (B_fast / B_ref); rows 0-2 are the velocity itself; finite
    wherever the value is and NaN exactly where it is NaN (rows 9-11 at rest, nothing else); exact zeros where the NaN reset zeroes
    a whole component, and -- reference order -- wherever the value is an exact zero (tanh saturated: 1 - 1).  The throughput form
    has no saturation; its far field is an exact zero once exp underflows, asserted for the single-obstacle samples at |h| >= 400."""
    bound = "Bfast" if flavour == "fast" else "Bref"
    rhs = evaluate(ctx, flavour)[0]
    got = rhs[:, 3:12]
    idx = np.flatnonzero(FIX["dec"])
    r = ratios(got, FIX["val"], FIX[bound])
    with capsys.disabled():
        print()
        report("%s rhs/%s rows 3-11" % (flavour, bound), idx, r[idx])
    assert np.array_equal(rhs[:, 0:3], FIX["X"][:, 3:6])
    assert np.array_equal(np.isnan(got), np.isnan(FIX["val"])) and not np.isinf(got).any()
    assert np.all(got[:, MAPPED9][FIX["reset"]] == 0)
    if flavour == "fast":
        far = np.abs(FIX["h_ray"]) >= 400
        assert far.sum() >= 20 and np.all(got[far][FIX["val"][far] == 0] == 0)
    else:
        assert np.all(got[FIX["val"] == 0] == 0)
    assert np.all(r[idx] <= 1.0), np.argwhere(r[idx] > 1.0)[:8]


def test_reference_order_plain_rows_bit_equal(ctx):
    """Rows 0-5, 9-11 and the control of the reference-order flavour hold no tanh: equal to the reference's own doubles on every row,
    the alphaV != 0 blocks in particular."""
    rhs, ctl, _ = evaluate(ctx, "reference-order")
    assert np.array_equal(rhs[:, 3:12][:, PLAIN9], FIX["ref64_rhs"][:, PLAIN9], equal_nan=True)
    assert np.array_equal(ctl, FIX["ref64_u"])
    assert (FIX["blocks"][FIX["block"], 3] != 0).sum() >= 200


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_undecidable_rows_lie_on_an_adjacent_branch(ctx, flavour):
    bound = "Bfast" if flavour == "fast" else "Bref"
    und = FIX["und"]
    assert len(und)
    got = evaluate(ctx, flavour)[0][und, 3:12]
    here = ratios(got, FIX["val"][und], FIX[bound][und])
    there = ratios(got, FIX["alt_val"], FIX["alt_" + bound])
    assert np.all(np.minimum(here, there) <= 1.0), np.argwhere(np.minimum(here, there) > 1.0)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_control_and_hamiltonian_within_bound(ctx, flavour, capsys):
    """Both flavours evaluate the control and the Hamiltonian by the reference-order expressions (the throughput flavour under
    contraction: fewer roundings than the bound counts); the throughput flavour's Hamiltonian reads map_fast<F>, so its map term
    takes that form's bound (BHfast).  An undecidable row may sit on either branch."""
    _, u, h = evaluate(ctx, flavour)
    bh = "BHfast" if flavour == "fast" else "BH"
    ru, rh = ratios(u, FIX["u"], FIX["Bu"]), ratios(h, FIX["H"], FIX[bh])
    und = FIX["und"]
    ru[und] = np.minimum(ru[und], ratios(u[und], FIX["alt_u"], FIX["alt_Bu"]))
    rh[und] = np.minimum(rh[und], ratios(h[und], FIX["alt_H"], FIX["alt_" + bh]))
    with capsys.disabled():
        print()
        report("%s control/B_u" % flavour, np.arange(N), ru)
        report("%s hamiltonian/%s" % (flavour, bh), np.arange(N), rh[:, None])
    assert np.all(np.isfinite(u)) and np.all(np.isfinite(h))
    assert np.all(ru <= 1.0), np.argwhere(ru > 1.0)[:8]
    assert np.all(rh <= 1.0), np.flatnonzero(rh > 1.0)[:8]


def one_batch(ctx, flavour, table, P, X):
    """(rhs, control, H) of the rows X as ONE eval_batch each, under one map and one parameter block."""
    from socp_amd import capi
    ctx.set_variant(_variant(flavour))
    try:
        ctx.set_map(table)
        ctx.set_params(P)
        return tuple(ctx.eval_batch(what, 0.0, X) for what in (capi.EVAL_RHS, capi.EVAL_CONTROL, capi.EVAL_HAMILTONIAN))
    finally:
        ctx.set_variant(capi.VARIANT_AUTO)


@pytest.mark.parametrize("B", [1, 63, 64, 65])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_rows_do_not_depend_on_the_batch(ctx, flavour, B):
    """Every lane reads one table through the scalar cache: the first B rows, alone, are bit-equal to the same rows of the whole
    batch, below, at and past one 64-lane wave.  Shipped map: the 256 points of the nominal group, all under the first point's
    parameter block, so that the whole batch spans four waves; the points the fixture holds under that block are, in this batch,
    also bit-equal to what the bound tests judged (evaluated there in a batch of their own).  256-obstacle map (the longest
    sequential sum): 80 points moved inside the grid."""
    nominal = np.flatnonzero((FIX["group"] == GROUPS.index("nominal")) & (FIX["map"] == MAPS.index("shipped")))
    b = FIX["block"][nominal[0]]
    grid = FIX["X"][:80].copy()
    grid[:, 0:3] = np.abs(grid[:, 0:3]) % 64.0 + 1.0 / 128
    whole = {}
    for name, X in (("shipped", FIX["X"][nominal]), ("grid256", grid)):
        assert len(X) > 65 and len(X[:B]) == B
        whole[name] = one_batch(ctx, flavour, FIX["table_" + name], FIX["blocks"][b], X)
        part = one_batch(ctx, flavour, FIX["table_" + name], FIX["blocks"][b], X[:B])
        for p, w in zip(part, whole[name]):
            assert len(p) == B and np.all(np.isfinite(w)) and np.array_equal(p, w[:B])
    own = np.flatnonzero(FIX["block"][nominal] == b)
    assert len(own) >= 16
    rhs, ctl, ham = evaluate(ctx, flavour)
    for w, judged in zip(whole["shipped"], (rhs, ctl, ham[:, None])):
        assert np.array_equal(w[own], judged[nominal[own]])


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_segment_against_mpf_rk4(ctx, flavour, capsys):
    """100 RK4 steps from 64 starts on the shipped map (muObs = 0.3, ca = 0.05, alphaV = 0.05) against the same recurrence in mpf on
    the mathematical right-hand side.  The yardstick is the REFERENCE's own deviation from the mpf trajectory (its ModelInt, stored
    per component as the batch maximum): either flavour stays within 8x that figure plus 8 u |X|."""
    from socp_amd import capi
    ctx.set_map(FIX["table_shipped"])
    ctx.set_params(FIX["traj_P"])
    ctx.set_step_number(int(FIX["traj_N"]))
    ctx.set_variant(_variant(flavour))
    try:
        Xf = ctx.integrate_batch(0.0, float(FIX["traj_tf"]), FIX["traj_X0"])
    finally:
        ctx.set_variant(capi.VARIANT_AUTO)
    ref, dev = FIX["traj_mpf"], FIX["traj_ref_dev"]
    err = np.abs(Xf - ref)
    allowed = 8 * dev[None, :] + 8 * U * np.abs(ref)
    with capsys.disabled(), np.errstate(all="ignore"):
        print()
        print("segment: reference deviation per component:        %s" % " ".join("%.2e" % v for v in dev))
        print("segment: %s deviation per component: %s" % (flavour, " ".join("%.2e" % v for v in err.max(axis=0))))
        print("segment: %s err/allowed per component: %s" % (flavour, " ".join("%.3f" % v for v in (err / allowed).max(axis=0))))
    assert np.all(np.isfinite(Xf))
    assert np.all(err <= allowed), np.argwhere(err > allowed)[:8]
