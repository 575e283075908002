"""GPU: the throughput flavour's right-hand sides (socp_amd/csrc/models_fast.hpp) pinned row by row and component by component to
a 240-bit evaluation, within a bound that carries each component's conditioning (tests/fast_reference.py; the fixture
tests/golden/fast_pin.npz is written by tests/golden/make_fast_golden.py and checked on the CPU by tests/test_fast_pin_cpu.py).

Every evaluation goes through capi.Context.eval_batch with per-row t and switching times, one call per parameter block.  The
bounds are derived (running error analysis, the primitives' budgets 2u each); the ratios these tests print are observations
(profiles/fast_pin_gpu_tests.txt) and none of them is a tolerance.

Control and Hamiltonian: GoddardFastT delegates both to the reference-order code, but in the translation unit that is compiled
with contraction (models_fast.hpp says so), so the design does NOT intend bit equality with the reference-order flavour -- its
products and sums fuse.  They are therefore held to the Tracked bound of the reference-order expressions (a fused multiply-add
has fewer roundings than the two operations the bound counts)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "fast_pin.npz"))
GROUPS = [str(g) for g in FIX["group_names"]]
U = 2.0 ** -53


@pytest.fixture(scope="module")
def ctxs():
    from socp_amd import capi
    c = {"g_": capi.Context(capi.MODEL_GODDARD), "c_": capi.Context(capi.MODEL_COVID19)}
    yield c
    for v in c.values():
        v.close()


_cache = {}


def evaluate(ctxs, p, variant, what, rows=None):
    """eval_batch over the fixture's rows (all, or the index array `rows`), one call per parameter block; cached per flavour."""
    from socp_amd import capi
    key = (p, variant, what)
    if rows is None and key in _cache:
        return _cache[key]
    c = ctxs[p]
    idx = np.arange(len(FIX[p + "X"])) if rows is None else np.asarray(rows)
    out = None
    c.set_variant(variant)
    try:
        for b, P in enumerate(FIX[p + "blocks"]):
            sel = idx[FIX[p + "block"][idx] == b]
            if not len(sel):
                continue
            c.set_params(P)
            r = c.eval_batch(what, FIX[p + "t"][sel], FIX[p + "X"][sel], sw=FIX[p + "sw"][sel])
            if out is None:
                out = np.full((len(FIX[p + "X"]), r.shape[1]), np.nan)
            out[sel] = r
    finally:
        c.set_variant(capi.VARIANT_AUTO)
    if rows is None:
        out.setflags(write=False)
        _cache[key] = out
        return out
    return out[idx]


def ratios(got, val, B):
    err = np.abs(got - val)
    with np.errstate(all="ignore"):
        return np.where(err == 0, 0.0, err / B)


def report(title, p, idx, r):
    for g in sorted(set(FIX[p + "group"][idx])):
        sel = FIX[p + "group"][idx] == g
        print("%s %-14s max err/B per component: %s" % (title, GROUPS[g], " ".join("%.3f" % v for v in np.atleast_2d(r[sel]).max(axis=0))))


def _flavours():
    from socp_amd import capi
    return {"fast": (capi.VARIANT_LANE_FAST, "Bfast"), "reference-order": (capi.VARIANT_LANE_EXACT, "Bref")}


@pytest.mark.parametrize("flavour", ["fast", "reference-order"])
@pytest.mark.parametrize("p", ["g_", "c_"], ids=["goddard", "covid"])
def test_rhs_within_bound(ctxs, p, flavour, capsys):
    """Decidable rows of every group: |rhs - value| <= B per component (B_fast for the throughput flavour, B_ref for the
    reference-order kernel), and finite wherever the oracle's value is (the fixture's values all are)."""
    from socp_amd import capi
    variant, bound = _flavours()[flavour]
    got = evaluate(ctxs, p, variant, capi.EVAL_RHS)
    idx = np.flatnonzero(FIX[p + "dec"])
    finite = np.isfinite(FIX[p + "val"][idx])
    r = ratios(got[idx], FIX[p + "val"][idx], FIX[p + bound][idx])
    with capsys.disabled():
        print()
        report("%s rhs/%s" % (flavour, bound), p, idx, r)
    assert np.all(np.isfinite(got[idx][finite]))
    assert np.all(r[finite] <= 1.0), np.argwhere(r > 1.0)[:8]


@pytest.mark.parametrize("flavour", ["fast", "reference-order"])
@pytest.mark.parametrize("p", ["g_", "c_"], ids=["goddard", "covid"])
def test_undecidable_rows_lie_on_an_adjacent_branch(ctxs, p, flavour):
    """Rows too close to a kink to say which branch a correct evaluation takes: each component is within its bound of the value of
    one of the two adjacent branches (both stored)."""
    from socp_amd import capi
    variant, bound = _flavours()[flavour]
    und = FIX[p + "und"]
    assert len(und)
    got = evaluate(ctxs, p, variant, capi.EVAL_RHS)[und]
    here = ratios(got, FIX[p + "val"][und], FIX[p + bound][und])
    there = ratios(got, FIX[p + "alt_val"], FIX[p + "alt_" + bound])
    assert np.all(np.isfinite(got))
    assert np.all(np.minimum(here, there) <= 1.0), np.argwhere(np.minimum(here, there) > 1.0)


def test_fast_control_and_hamiltonian_within_reference_order_bound(ctxs, capsys):
    """See the module docstring: contraction on, so a bound and not bit equality.  All Goddard rows; an undecidable row may sit on
    either branch."""
    from socp_amd import capi
    u = evaluate(ctxs, "g_", capi.VARIANT_LANE_FAST, capi.EVAL_CONTROL)
    h = evaluate(ctxs, "g_", capi.VARIANT_LANE_FAST, capi.EVAL_HAMILTONIAN)[:, 0]
    ru = ratios(u, FIX["g_u"], FIX["g_Bu"])
    rh = ratios(h, FIX["g_H"], FIX["g_BH"])
    und = FIX["g_und"]
    ru[und] = np.minimum(ru[und], ratios(u[und], FIX["g_alt_u"], FIX["g_alt_Bu"]))
    rh[und] = np.minimum(rh[und], ratios(h[und], FIX["g_alt_H"], FIX["g_alt_BH"]))
    idx = np.arange(len(u))
    with capsys.disabled():
        print()
        report("fast control/B_u", "g_", idx, ru)
        report("fast hamiltonian/B_H", "g_", idx, rh[:, None])
    assert np.all(np.isfinite(u)) and np.all(np.isfinite(h))
    assert np.all(ru <= 1.0), np.argwhere(ru > 1.0)[:8]
    assert np.all(rh <= 1.0), np.flatnonzero(rh > 1.0)[:8]
    # the reference-order flavour, the same expressions without contraction, meets the same bound
    ue = evaluate(ctxs, "g_", capi.VARIANT_LANE_EXACT, capi.EVAL_CONTROL)
    assert np.all(ratios(ue, FIX["g_u"], FIX["g_Bu"])[FIX["g_dec"]] <= 1.0)


@pytest.mark.parametrize("B", [1, 63, 64, 65])
def test_rows_do_not_depend_on_the_batch(ctxs, B):
    """The nominal group, per parameter block, as its first B rows and whole: bit-equal rows however they are batched."""
    from socp_amd import capi
    whole = evaluate(ctxs, "g_", capi.VARIANT_LANE_FAST, capi.EVAL_RHS)
    nominal = np.flatnonzero(FIX["g_group"] == GROUPS.index("nominal"))
    for b in sorted(set(FIX["g_block"][nominal])):
        sel = nominal[FIX["g_block"][nominal] == b][:B]
        part = evaluate(ctxs, "g_", capi.VARIANT_LANE_FAST, capi.EVAL_RHS, rows=sel)
        assert np.array_equal(part, whole[sel], equal_nan=True), b
    mu2_1 = nominal[FIX["g_blocks"][FIX["g_block"][nominal], 6] == 1.0]
    assert len(mu2_1) >= 65 or B < 65


def test_short_segment_against_mpf_rk4(ctxs, capsys):
    """N = 10 RK4 steps from 64 starts against the same recurrence in mpf on the mathematical right-hand side.  No bound has been
    derived for this; the yardstick is the reference-order CPU oracle's own deviation from the mpf trajectory (stored per component
    as the batch maximum): two double-precision runs of one recurrence differ from the exact one by comparable amounts, so the
    throughput flavour has to stay within 8x that figure plus 8 u |X|."""
    from socp_amd import capi
    c = ctxs["g_"]
    c.set_params(FIX["traj_P"])
    c.set_step_number(int(FIX["traj_N"]))
    c.set_variant(capi.VARIANT_LANE_FAST)
    try:
        Xf = c.integrate_batch(0.0, float(FIX["traj_tf"]), FIX["traj_X0"])
    finally:
        c.set_variant(capi.VARIANT_AUTO)
    ref, dev = FIX["traj_mpf"], FIX["traj_oracle_dev"]
    err = np.abs(Xf - ref)
    allowed = 8 * dev[None, :] + 8 * U * np.abs(ref)
    with capsys.disabled(), np.errstate(all="ignore"):
        print()
        print("segment: oracle deviation per component: %s" % " ".join("%.2e" % v for v in dev))
        print("segment: fast deviation per component:   %s" % " ".join("%.2e" % v for v in err.max(axis=0)))
        print("segment: fast err/allowed per component: %s" % " ".join("%.3f" % v for v in (err / allowed).max(axis=0)))
    assert np.all(np.isfinite(Xf))
    assert np.all(err <= allowed), np.argwhere(err > allowed)[:8]
