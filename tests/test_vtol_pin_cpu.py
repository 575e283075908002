"""CPU: the instrument that pins vtolUAV's right-hand sides (tests/vtol_reference.py, tests/golden/vtol_pin.npz) is itself checked
before any kernel is judged by it.

  * the reference-order restatement, in numpy.float64, equals the REFERENCE's own numbers (ref64_*, produced by the reference's
    objects) bit for bit in every row without tanh and in the control, and lies within B_ref of them in rows 6-8 and H -- on every
    row, the alphaV != 0 blocks, the ellipsoid's quirks, the resets and the NaN rows included.  This ties the restatement to the
    reference and not to the kernel;
  * the fixtures of vtol_vectors.npz are reproduced under the same rule;
  * the reference's numbers lie within B_ref of the 240-bit value on every decidable row (on an undecidable one: of one of the two
    adjacent branches), the throughput structure emulated in numpy.float64 within B_fast;
  * six deliberately wrong emulations each VIOLATE B_fast on a decidable row; two of them (an inexact rsqrt, a sign flipped in a
    non-nearest box away from it) pass the old bar of tests/test_gpu_vtol.py on the whole nominal group -- the bound sees what
    that bar cannot; that two others (the same flip in an abutting box, `pos` inverted) are visible to the old bar already is
    asserted as well;
  * at least 95 % of every group but `kinks` is decidable;
  * with mpmath present, a sample of rows evaluated afresh equals the stored fixture bit for bit."""
import functools
import os
import sys

import numpy as np
import pytest

import fast_reference as fr
import vtol_reference as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "vtol_pin.npz"))
V = np.load(os.path.join(ROOT, "tests", "golden", "vtol_vectors.npz"))
GROUPS = [str(g) for g in FIX["group_names"]]
MAPS = [str(m) for m in FIX["map_names"]]
N = len(FIX["X"])
SUB = list(range(3, 12))                # the stored rows of the right-hand side; rows 0-2 are X[3:6] themselves
PLAIN9 = [0, 1, 2, 6, 7, 8]             # within the stored nine: rows 3-5 and 9-11 (no map, no tanh)
MAPPED9 = [3, 4, 5]                     # rows 6-8


def row(i):
    return FIX["blocks"][FIX["block"][i]], FIX["table_" + MAPS[FIX["map"][i]]], FIX["X"][i]


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


@functools.lru_cache(maxsize=None)
def emulation(form, mutation=None, rsqrt_error=0.0):
    """Every row of the fixture through one restatement in numpy.float64: (rhs[N, 9], u[N, 3], H[N])."""
    kit = {}
    if mutation:
        kit["mutation"] = mutation
    if rsqrt_error:
        kit["rsqrt"] = lambda x: (np.float64(1.0) / np.sqrt(x)) * np.float64(1.0 + rsqrt_error)
    fn = {"ref": vr.vtol_ref, "fast": vr.vtol_fast}[form]
    d, u, H = np.empty((N, 9)), np.empty((N, 3)), np.empty(N)
    for i in range(N):
        full, u[i], H[i] = vr.emulate(fn, *row(i), **kit)
        assert np.array_equal(full[0:3], FIX["X"][i, 3:6])
        d[i] = full[SUB]
    return d, u, H


def test_fixture_shape_and_decidable_share():
    assert set(GROUPS[g] for g in FIX["group"]) == set(GROUPS) and set(MAPS[m] for m in FIX["map"]) == set(MAPS)
    assert np.array_equal(np.flatnonzero(~FIX["dec"]), FIX["und"]) and len(FIX["und"])
    for g, name in enumerate(GROUPS):
        share = FIX["dec"][FIX["group"] == g].mean()
        print("%-16s %4d rows, %.1f %% decidable" % (name, (FIX["group"] == g).sum(), 100 * share))
        assert name == "kinks" or share >= 0.95, name
    P = FIX["blocks"][FIX["block"]]
    for index, values in ((vr.I_ALPHAV, (0.05, 2)), (vr.I_VD, (1, 0.25)), (vr.I_AMAX, (0.3, 3)), (vr.I_PHIOBS, (1, 40)), (vr.I_ALPHAT, (0.05, 1)),
                          (vr.I_CA, (0, 0.05))):
        assert set(values) <= set(P[FIX["group"] == GROUPS.index("parameters"), index])
    par = FIX["group"] == GROUPS.index("parameters")
    speed = np.linalg.norm(FIX["X"][par, 3:6], axis=1)
    for Vd in (1, 0.25):
        on = P[par, vr.I_VD] == Vd
        assert np.any(speed[on] > Vd) and np.any(speed[on] < Vd)
    assert speed.min() < 1.1e-3
    assert len(FIX["table_grid256"]) == 256 and len(FIX["table_empty"]) == 0
    kinks = FIX["group"] == GROUPS.index("kinks")
    assert FIX["reset"][kinks].any(axis=0).all() and np.isnan(FIX["val"][kinks][:, 6:9]).all(axis=1).sum() >= 3
    assert not np.isnan(FIX["val"][:, 0:6]).any() and not np.isnan(FIX["val"][~kinks]).any()
    assert np.all(FIX["h_ray"][kinks & ~np.isnan(FIX["h_ray"])] == 0)          # the samples on the surface itself are kept as kink rows
    h = FIX["h_ray"][(FIX["group"] == GROUPS.index("single_obstacle")) | kinks]
    assert {0.0, 2.0 ** -30, -0.5, 355.0, -365.0, 372.0, 400.0, 4000.0, -4000.0} <= set(h)


def test_reference_order_restatement_equals_the_reference(capsys):
    d, u, H = emulation("ref")
    assert np.array_equal(d[:, PLAIN9], FIX["ref64_rhs"][:, PLAIN9], equal_nan=True)
    assert np.array_equal(np.isnan(d), np.isnan(FIX["val"]))                      # NaN in the same components, nothing else
    assert np.array_equal(u, FIX["ref64_u"])
    r = ratios(d[:, MAPPED9], FIX["ref64_rhs"][:, MAPPED9], FIX["Bref"][:, MAPPED9])
    rh = ratios(H, FIX["ref64_H"], FIX["BH"])
    with capsys.disabled():
        print()
        report("restatement - reference / B_ref, rows 6-8", np.arange(N), r)
        report("restatement - reference / B_H", np.arange(N), rh[:, None])
    assert np.all(r <= 1.0), np.argwhere(r > 1.0)[:5]
    assert np.all(rh <= 1.0), np.flatnonzero(rh > 1.0)[:5]
    nonzero_alphaV = FIX["blocks"][FIX["block"], vr.I_ALPHAV] != 0
    assert nonzero_alphaV.sum() >= 200


def test_existing_fixtures_reproduced():
    """vtol_vectors.npz (written by make_vtol_golden.py from the reference) under the same rule.  The nominal and near-surface groups
    ARE its points, in its order, shipped map first; the extreme points have no row here and get their bound in-process."""
    d, u, H = emulation("ref")
    nom = np.flatnonzero(FIX["group"] == GROUPS.index("nominal"))
    near = np.flatnonzero(FIX["group"] == GROUPS.index("near_surface"))
    n, m = len(V["X"]), len(V["near_X"])
    assert len(nom) == 2 * n and len(near) == 2 * m and np.array_equal(FIX["X"][nom[:n]], V["X"]) and np.array_equal(FIX["X"][near[m:]], V["near_X"])
    for idx, plain, ctl, g, ham in ((nom[:n], V["rhs_3_12"][:, PLAIN9], V["ctl"], V["rhs_3_12"][:, 3:6], V["ham"]),
                                    (nom[n:], V["rhs_3_12"][:, PLAIN9], V["ctl"], V["syn_rhs_6_9"], V["syn_ham"]),
                                    (near[:m], V["near_rhs_plain"][:, 3:9], V["near_ctl"], V["near_rhs_6_9"], V["near_ham"]),
                                    (near[m:], V["near_rhs_plain"][:, 3:9], V["near_ctl"], V["near_syn_rhs_6_9"], V["near_syn_ham"])):
        assert np.array_equal(d[idx][:, PLAIN9], plain) and np.array_equal(u[idx], ctl)
        assert np.all(ratios(d[idx][:, MAPPED9], g, FIX["Bref"][idx][:, MAPPED9]) <= 1.0)
        assert np.all(ratios(H[idx], ham, FIX["BH"][idx]) <= 1.0)
    for k in range(len(V["ext_X"])):
        full, uk, Hk = vr.emulate(vr.vtol_ref, V["ext_params"][k], V["table_shipped"], V["ext_X"][k])
        assert np.array_equal(full[vr.PLAIN], V["ext_rhs"][k, vr.PLAIN]) and np.array_equal(uk, V["ext_ctl"][k])
        if fr.HAVE_MPMATH:
            e = vr.evaluate_row(V["ext_params"][k], V["table_shipped"], V["ext_X"][k])
            assert np.all(ratios(full[vr.MAPPED], V["ext_rhs"][k, vr.MAPPED], e["B_ref"][vr.MAPPED]) <= 1.0)
            assert ratios(Hk, V["ext_ham"][k], e["B_H"]) <= 1.0
            assert np.all(full[vr.MAPPED][e["reset"]] == 0)


def test_reference_within_b_ref(capsys):
    idx = np.flatnonzero(FIX["dec"])
    r = ratios(FIX["ref64_rhs"], FIX["val"], FIX["Bref"])
    ru = ratios(FIX["ref64_u"], FIX["u"], FIX["Bu"])
    rh = ratios(FIX["ref64_H"], FIX["H"], FIX["BH"])
    with capsys.disabled():
        print()
        report("reference/B_ref", idx, r[idx])
        report("reference control/B_u", idx, ru[idx])
        report("reference H/B_H", idx, rh[idx][:, None])
    und = FIX["und"]
    r[und] = np.minimum(r[und], ratios(FIX["ref64_rhs"][und], FIX["alt_val"], FIX["alt_Bref"]))
    ru[und] = np.minimum(ru[und], ratios(FIX["ref64_u"][und], FIX["alt_u"], FIX["alt_Bu"]))
    rh[und] = np.minimum(rh[und], ratios(FIX["ref64_H"][und], FIX["alt_H"], FIX["alt_BH"]))
    assert np.all(r <= 1.0), np.argwhere(r > 1.0)[:5]
    assert np.all(ru <= 1.0) and np.all(rh <= 1.0)
    assert np.all(FIX["ref64_rhs"][:, MAPPED9][FIX["reset"]] == 0) and np.all(FIX["Bref"][:, MAPPED9][FIX["reset"]] == 0)


def test_float64_emulation_of_the_throughput_form_within_b_fast(capsys):
    d, u, H = emulation("fast")
    idx = np.flatnonzero(FIX["dec"])
    r = ratios(d, FIX["val"], FIX["Bfast"])[idx]
    ru = ratios(u, FIX["u"], FIX["Bu"])[idx]
    rh = ratios(H, FIX["H"], FIX["BHfast"])[idx]
    with capsys.disabled():
        print()
        report("float64/B_fast", idx, r)
        report("float64 H/B_H_fast", idx, rh[:, None])
    assert np.all(r <= 1.0), np.argwhere(r > 1.0)[:5]
    assert np.all(ru <= 1.0) and np.all(rh <= 1.0)


def old_bar(d, u, H):
    """The throughput flavour's bar in tests/test_gpu_vtol.py on the nominal group: max |d| / max(1, |ref|), against the reference."""
    nom = FIX["group"] == GROUPS.index("nominal")
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))
    return max(rel(d[nom], FIX["ref64_rhs"][nom]), rel(u[nom], FIX["ref64_u"][nom]), rel(H[nom], FIX["ref64_H"][nom]))


MUTATIONS = {
    "rsqrt with relative error 1e-11": dict(rsqrt_error=1e-11),
    "sign of g1 flipped for the second-nearest box": dict(mutation="g1_second_nearest"),
    "sign of g1 flipped for the second-nearest box where it is 12 muObs away or more": dict(mutation="g1_second_nearest_far"),
    "pos selection inverted for |h| > 20": dict(mutation="pos_far"),
    "the ellipsoid gradient's rad with its z term": dict(mutation="zterm"),
    "+w*v in rows 9-11": dict(mutation="w_sign"),
}
# the defects the old bar of tests/test_gpu_vtol.py (1e-8 of max(1, |ref|)) cannot see, by construction: a relative 1e-11 on
# quantities of size <= 10, and a term of at most phiObs (2 / muObs) (1/4) exp(-2 * 12) = 3.8e-10 at muObs = 0.05 taken twice
BELOW_THE_OLD_BAR = ["rsqrt with relative error 1e-11", "sign of g1 flipped for the second-nearest box where it is 12 muObs away or more"]
VISIBLE_TO_THE_OLD_BAR = ["sign of g1 flipped for the second-nearest box", "pos selection inverted for |h| > 20"]


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_mutations_violate_b_fast(name, capsys):
    """Each wrong emulation leaves B_fast (or B_H_fast) on at least one decidable row; the unmutated one on none.  Printed beside
    it: what the old bar makes of the same emulation on the nominal group.  Measured: 1.0e-11 (rsqrt), 2.3e-3 (second-nearest box,
    anywhere), 8.3e-11 (second-nearest box, 12 muObs away or more), 9.1 (pos inverted), 0.12 (z term: the synthetic map's ellipsoids), 9.8e-16
    (w: alphaV = 0 in that group).  So two of them are NOT below the old bar on every nominal point, although the issue that asked for
    this instrument supposed so: the shipped boxes abut, and at 7 of the 512 nominal rows (all at muObs = 1) the second-nearest
    box's g1 term exceeds 1e-8; and m = q ~ 1 in place of e q ~ 4e-18, or the reverse, switches a box on or off wherever ONE axis
    is 20 muObs from its face whatever the other two do (231 of the 512 rows, 489 in H).  The far-box variant is the sign flip
    confined to where the old bar cannot see it."""
    good, bad = emulation("fast"), emulation("fast", **MUTATIONS[name])
    dec = FIX["dec"]
    both = lambda e: np.concatenate([ratios(e[0], FIX["val"], FIX["Bfast"]), ratios(e[2], FIX["H"], FIX["BHfast"])[:, None]], axis=1)[dec]
    r = both(bad)
    with capsys.disabled():
        print("\n%s: rows beyond B_fast %d of %d, largest err/B %.3g; old bar on the nominal group %.3e (unmutated %.3e)"
              % (name, (r > 1.0).any(axis=1).sum(), dec.sum(), r[np.isfinite(r)].max(), old_bar(*bad), old_bar(*good)))
    assert np.all(both(good) <= 1.0)
    assert np.any(r > 1.0)


@pytest.mark.parametrize("name", BELOW_THE_OLD_BAR)
def test_the_instrument_sees_what_the_old_bar_cannot(name):
    """These emulations pass the old bar on the WHOLE nominal group (and test_mutations_violate_b_fast shows each leaves B_fast)."""
    assert old_bar(*emulation("fast")) <= 1e-8
    assert old_bar(*emulation("fast", **MUTATIONS[name])) <= 1e-8


@pytest.mark.parametrize("name", VISIBLE_TO_THE_OLD_BAR)
def test_what_the_old_bar_sees_already(name):
    """The issue that asked for this instrument supposed these two below the old bar on the whole nominal group.  They are not
    (test_mutations_violate_b_fast's docstring has the figures and the reason); asserted, so that the statement stays true of
    the fixture as it is."""
    assert old_bar(*emulation("fast", **MUTATIONS[name])) > 1e-8


@pytest.mark.skipif(not fr.HAVE_MPMATH, reason="the generator's arithmetic (mpmath) is not installed")
def test_sample_rows_regenerate_bit_for_bit():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_vtol_pin_golden as gen
    small = np.flatnonzero(FIX["map"] != MAPS.index("grid256"))
    idx = np.unique(np.concatenate([small[np.linspace(0, len(small) - 1, gen.REGEN_ROWS - 1).astype(int)],
                                    np.flatnonzero(FIX["map"] == MAPS.index("grid256"))[:1]]))
    for stored, fresh in gen.regenerate(FIX, idx):
        assert np.array_equal(np.asarray(stored), np.asarray(fresh, dtype=np.asarray(stored).dtype), equal_nan=True)
