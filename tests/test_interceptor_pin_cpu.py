"""CPU: the interceptor's pins (tests/golden/interceptor_pin.npz, written by tests/golden/make_interceptor_pin_golden.py).

Part A -- the C oracle (oracle/interceptor_oracle.c) equals the REFERENCE's own doubles BIT FOR BIT on every fixture row: the
reference's interceptor.cpp compiled as it lies against oracle/eigen_shim (both are g++ / libm without contraction).  Right-hand side,
control and Hamiltonian in both charts and both stages (ComputeMass on either side of t1 and at t1, with either flag), the new angles
and costates of both chart changes, trajectories with and without a chart change, the overridden final rows, the analytical guess.
Through a chart change the pin holds up to Eigen's summation order, which the shim stands in for.  Both sides of the comparison are
built with sin() and cos() as the texts call them (oracle/Makefile: NOFUSE): left alone, the compiler fuses some pairs into glibc's
sincos(), which is not bit-equal to sin() / cos() for ~0.07 % of arguments, and fuses different pairs on the two sides -- the one
row in this fixture that the default builds disagreed on (a chart change, three costates by one or two units in the last place) was
exactly that, and neither text departs from interceptor.cpp.  The default build of the oracle is held to the same rows within 1e-13.

Part B -- the instrument that pins both device flavours to a 240-bit evaluation (tests/interceptor_reference.py) is itself checked
before any kernel is judged by it: the fixture's shape and shares, the reference's doubles within B_ref, a float64 emulation of the
throughput form within B_fast, sample rows regenerated bit for bit, and wrong emulations that each leave the bound."""
import functools
import os
import sys

import numpy as np
import pytest

import fast_reference as fr
import interceptor_reference as ir
from oracle.oracle import Oracle, MODEL_INTERCEPTOR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "interceptor_pin.npz"))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "interceptor_vectors.npz"))
GROUPS = [str(g) for g in FIX["group_names"]]
CC_GROUPS = [str(g) for g in FIX["cc_group_names"]]
N, NCC = len(FIX["X"]), len(FIX["cc_X"])
PLANAR = CC_GROUPS.index("planar")


def row(i):
    return FIX["blocks"][FIX["block"][i]], int(FIX["chart"][i]), int(FIX["stage"][i]), float(FIX["t"][i]), FIX["X"][i]


def ratios(got, val, B):
    """|got - val| / B per component; 0 where they are equal (a bound of zero demands equality)."""
    with np.errstate(all="ignore"):
        err = np.abs(got - val)
        return np.where(got == val, 0.0, np.where(np.isnan(err), np.inf, err / B))


def report(title, group, names, r):
    for g in sorted(set(group)):
        print("%s %-14s max err/B per component: %s" % (title, names[g], " ".join("%.3f" % v for v in np.atleast_2d(r[group == g]).max(axis=0))))


# ---- Part A ---------------------------------------------------------------------------------------------------------------

def oracle_for(block, step_nbr=None, pin_build=True):
    o = Oracle(MODEL_INTERCEPTOR, step_nbr=step_nbr, pin_build=pin_build)
    o.set_params(FIX["blocks"][block])
    return o


def test_oracle_right_hand_side_control_hamiltonian_equal_the_reference_bit_for_bit(built):
    oracles = [oracle_for(b) for b in range(len(FIX["blocks"]))]
    seen = set()
    for i in range(N):
        P, chart, stage, t, X = row(i)
        o = oracles[FIX["block"][i]]
        o.set_flags(chart, stage)
        assert np.array_equal(o.rhs(t, X), FIX["ref64_rhs"][i]), i
        assert np.array_equal(o.control(t, X), FIX["ref64_u"][i]), i
        assert o.hamiltonian(t, X)[0] == FIX["ref64_H"][i], i
        seen.add((chart, stage, np.sign(t - 20.0)))
    assert seen == {(c, s, d) for c in (1, 2) for s in (0, 1) for d in (-1.0, 0.0, 1.0)}     # ComputeMass: t < t1, == t1, > t1


def test_oracle_chart_changes_equal_the_reference_bit_for_bit(built):
    o = oracle_for(int(FIX["cc_block"]))
    for x, want12, want21 in zip(FIX["cc_X"], FIX["ref64_c12"], FIX["ref64_c21"]):
        assert np.array_equal(o.chart12(x), want12)
        assert np.array_equal(o.chart21(want12), want21)
    assert np.all(np.isfinite(FIX["ref64_c12"])) and np.all(np.isfinite(FIX["ref64_c21"]))      # the planar and vertical rows included


def test_default_build_of_the_oracle_differs_by_sincos_fusion_only(built):
    """libsocp_oracle.so (sin / cos pairs fused where the compiler chose to), the build every other test uses, on every pinned
    quantity: right-hand side, control, Hamiltonian, both chart changes, the trajectories and segments with the flags they leave,
    the final rows and the analytical guess.  Equal, or within a few units in the last place relative to the row's largest
    component: 1e-13 on single evaluations and through the 6x6 solve of a chart change, 1e-10 after 50 steps per stage (the bar
    tests/test_gpu_interceptor.py sets a trajectory)."""
    oracles = [oracle_for(b, pin_build=False) for b in range(len(FIX["blocks"]))]
    close = lambda got, want, tol=1e-13: np.max(np.abs(got - want)) <= tol * np.abs(want).max()
    for i in range(N):
        P, chart, stage, t, X = row(i)
        o = oracles[FIX["block"][i]]
        o.set_flags(chart, stage)
        assert close(o.rhs(t, X), FIX["ref64_rhs"][i]) and close(o.control(t, X), FIX["ref64_u"][i])
        assert abs(o.hamiltonian(t, X)[0] - FIX["ref64_H"][i]) <= 1e-13 * max(abs(FIX["ref64_H"][i]), np.abs(FIX["ref64_rhs"][i]).max())
    out = FIX["cc_group"] != CC_GROUPS.index("vertical")                                       # singular Jacobian: no such bar there
    for x, want12, want21 in zip(FIX["cc_X"][out], FIX["ref64_c12"][out], FIX["ref64_c21"][out]):
        assert close(oracles[2].chart12(x), want12) and close(oracles[2].chart21(want12), want21)
    o = oracles[0]
    for a, e, x, want, fl in zip(FIX["a_traj_t0"], FIX["a_traj_tf"], FIX["a_traj_X0"], FIX["a_traj_Xf"], FIX["a_traj_flags"]):
        assert close(o.traj(a, x, e), want, 1e-10) and tuple(o.flags()) == tuple(fl)
    o5 = oracle_for(0, step_nbr=int(FIX["seg_N"]), pin_build=False)
    for a, e, x, want in zip(FIX["seg_t0"], FIX["seg_tf"], FIX["seg_X0"], FIX["ref64_seg"]):
        assert close(o5.traj(a, x, e), want, 1e-10)
    for rin, want in zip(FIX["a_final_in"], FIX["a_final_out"]):
        o.set_flags(int(rin[0]), int(rin[1]))
        assert np.array_equal(o.final_rows(rin[9:21], rin[21:33], rin[3:9].astype(np.int32)), want[:6])
        assert abs(o.hamiltonian(rin[2], rin[9:21])[0] + o.params()[ir.MUT] - want[12]) <= 1e-13 * max(1.0, abs(want[12]))
    for rin, want in zip(FIX["a_init_in"], FIX["a_init_out"]):
        xi, xf = np.zeros(12), np.zeros(12)
        xi[:6], xf[:6] = rin[2:8], rin[8:14]
        o.set_flags(1, int(rin[1]))
        assert close(o.init_analytical(rin[0], xi, 40.0, xf), want)


def test_oracle_trajectories_equal_the_reference_bit_for_bit(built):
    o = oracle_for(0)
    for a, e, x, want, fl in zip(FIX["a_traj_t0"], FIX["a_traj_tf"], FIX["a_traj_X0"], FIX["a_traj_Xf"], FIX["a_traj_flags"]):
        assert np.array_equal(o.traj(a, x, e), want)
        assert tuple(o.flags()) == tuple(fl)
    assert {int(c) for c, _ in FIX["a_traj_flags"]} == {1, 2}                                   # with and without a chart change
    o5 = oracle_for(0, step_nbr=int(FIX["seg_N"]))
    for a, e, x, want in zip(FIX["seg_t0"], FIX["seg_tf"], FIX["seg_X0"], FIX["ref64_seg"]):
        assert np.array_equal(o5.traj(a, x, e), want)


def test_oracle_final_rows_and_analytical_guess_equal_the_reference_bit_for_bit(built):
    o = oracle_for(0)
    overridden = 0
    for rin, want in zip(FIX["a_final_in"], FIX["a_final_out"]):
        chart, stage, tf = int(rin[0]), int(rin[1]), rin[2]
        mode, Xtf, xd = rin[3:9].astype(np.int32), rin[9:21], rin[21:33]
        o.set_flags(chart, stage)
        rows = o.final_rows(Xtf, xd, mode)
        assert np.array_equal(rows, want[:6]) and np.array_equal(rows, want[6:12])
        assert o.hamiltonian(tf, Xtf)[0] + o.params()[ir.MUT] == want[12]
        overridden += mode[3] == 0 and rows[3] == Xtf[9]
    assert overridden >= 2                                                                      # the vertical-target heading row
    for rin, want in zip(FIX["a_init_in"], FIX["a_init_out"]):
        xi, xf = np.zeros(12), np.zeros(12)
        xi[:6], xf[:6] = rin[2:8], rin[8:14]
        o.set_flags(1, int(rin[1]))
        assert np.array_equal(o.init_analytical(rin[0], xi, 40.0, xf), want)


def test_existing_fixtures_reproduced(built):
    """interceptor_vectors.npz (frozen from the oracle while it was unpinned) is still what the oracle gives, and the reference-order
    restatement of interceptor_reference.py in float64 agrees with it to the last places (numpy's sin / cos are not libm's)."""
    o = Oracle(MODEL_INTERCEPTOR)
    for chart, X in ((1, GOLD["X1"]), (2, GOLD["X2"])):
        for stage, t in ((1, 3.0), (0, 27.0)):
            o.set_flags(chart, stage)
            key = "c%d_s%d" % (chart, stage)
            assert np.array_equal(np.array([o.rhs(t, x) for x in X]), GOLD["rhs_" + key])
            assert np.array_equal(np.array([o.control(t, x) for x in X]), GOLD["ctl_" + key])
            assert np.array_equal(np.array([o.hamiltonian(t, x)[0] for x in X]), GOLD["ham_" + key])
            for x, want in zip(X[:4], GOLD["rhs_" + key]):
                d, _, _ = ir.emulate_rhs("ref", ir.SHIPPED, chart, stage, t, x)
                assert np.max(np.abs(d - want)) <= 1e-13 * np.abs(want).max()
    assert np.array_equal(np.array([o.chart21(x) for x in GOLD["X2"]]), GOLD["chart21_of_X2"])
    for a, e, x, want, fl in zip(GOLD["traj_t0"], GOLD["traj_tf"], GOLD["traj_X0"], GOLD["traj_Xf"], GOLD["traj_flags"]):
        assert np.array_equal(o.traj(a, x, e), want) and tuple(o.flags()) == tuple(fl)


# ---- Part B: the fixture ------------------------------------------------------------------------------------------------------

def informative(val, B):
    return np.all(B <= 1e-10 * np.maximum(1.0, np.abs(val)), axis=1)


def test_fixture_shape_and_shares(capsys):
    assert set(GROUPS[g] for g in FIX["group"]) == set(GROUPS) and set(CC_GROUPS[g] for g in FIX["cc_group"]) == set(CC_GROUPS)
    assert np.array_equal(np.flatnonzero(~FIX["dec"]), FIX["und"])
    # Undecidable rows for every kink that double inputs can bring within 4x its error.  Right-hand side: the saturation (b2 > 0 and
    # stage == 1 compare exact values: error zero).  Chart change: the pivot choice (l == L makes the first column's two largest
    # entries equal in value), in both directions, and the sel: selection at a vertical state (2 -> 1).  The chart change's other
    # decisions cannot be made undecidable from double inputs: c1 s2 < 0 / c1 c2 > 0, |key| < eps with eps = 1e-18 and key > 0 have
    # margins of the size of a sine or cosine of a double, never below ~1e-17 unless exactly zero, against errors of ~1e-16 times
    # that margin; a1 == +-pi/2 and |cos a1| >= chartLimit at chartLimit = 2 compare inputs.
    assert len(FIX["und"]) and all("|u|-u_max" in str(n) for n in FIX["und_names"])
    assert set(GROUPS[g] for g in FIX["group"][FIX["und"]]) == {"control"}
    assert np.array_equal(np.flatnonzero(~FIX["cc_dec12"]), FIX["cc_und12"]) and np.array_equal(np.flatnonzero(~FIX["cc_dec21"]), FIX["cc_und21"])
    assert len(FIX["cc_und12"]) and all("pivot" in str(n) for n in FIX["cc_und12_names"])
    names21 = [str(FIX["cc_und21_names"][i]) for i in FIX["cc_und21"]]
    assert any("pivot" in n for n in names21) and any("sel:" in n for n in names21)
    assert len(FIX["alt_cc_val12"]) == len(FIX["cc_und12"]) and len(FIX["alt_cc_val21"]) == len(FIX["cc_und21"])
    tie = FIX["cc_group"] == CC_GROUPS.index("pivot_tie")
    assert tie.sum() >= 3 and np.all(FIX["cc_X"][tie, 4] == FIX["cc_X"][tie, 5]) and not FIX["cc_dec12"][tie].any() and not FIX["cc_dec21"][tie].any()
    assert len(FIX["und"]) <= 0.1 * N and len(FIX["cc_und12"]) <= 0.1 * NCC and len(FIX["cc_und21"]) <= 0.1 * NCC
    assert NCC <= 64 and len(FIX["seg_X0"]) == 4 and int(FIX["seg_N"]) == 5
    assert np.all(np.isfinite(FIX["val"])) and np.all(np.isfinite(FIX["Bref"])) and np.all(np.isfinite(FIX["Bfast"]))
    # every group in both charts and, but for the angle and costate groups, both stages; two parameter blocks in the nominal group
    for g, name in enumerate(GROUPS):
        sel = FIX["group"] == g
        assert set(FIX["chart"][sel]) == {1, 2}
        assert name in ("angles", "costates") or set(FIX["stage"][sel]) == {0, 1}
    nominal = FIX["group"] == GROUPS.index("nominal")
    assert len(set(FIX["block"][nominal])) >= 2 and np.any(FIX["t"][nominal] == 20.0)
    P1 = FIX["blocks"][1]
    assert P1[ir.MU_GFT] == 0.6 and P1[ir.MUC] != 0
    c1 = np.abs(np.cos(FIX["X"][FIX["group"] == GROUPS.index("near_limit"), 2]))
    assert c1.min() < 2e-6 and np.any((c1 > 0.1) & (c1 < 0.1002)) and np.any((c1 < 0.1) & (c1 > 0.0998))
    a2 = FIX["X"][FIX["group"] == GROUPS.index("angles"), 3]
    assert {3.0, -3.0, np.pi, -np.pi, np.pi / 2, -np.pi / 2, 100.0, -100.0, 1e4, -1e4} <= set(a2) and np.abs(FIX["X"][:, 2:6]).max() <= ir.SINCOS_FAST_RANGE
    pa = np.abs(FIX["X"][FIX["group"] == GROUPS.index("costates"), 8])
    assert pa.min() <= 1e-170 and pa.max() >= 1e160
    ctl = FIX["group"] == GROUPS.index("control")
    assert np.any(np.abs(FIX["u"][ctl, 0]) < 0.6) and np.any(FIX["u"][ctl, 0] == 1.0) and np.any(FIX["u"][ctl, 0] == -1.0)
    assert np.any(np.all(FIX["X"][ctl, 8:10] == 0, axis=1)) and np.any(np.abs(FIX["u"][ctl, 1]) == np.pi)       # beta = +-pi: p_a2 = +-0.0
    assert {np.pi, -np.pi} <= set(FIX["u"][ctl, 1])
    # the right-hand side's bound, relative to the row's largest component: 1e-11 everywhere (the near-limit and costate groups are
    # exempt by the issue's letter and meet it all the same)
    with capsys.disabled():
        print()
        for bound in ("Bref", "Bfast"):
            rel = FIX[bound].max(axis=1) / np.abs(FIX["val"]).max(axis=1)
            for g, name in enumerate(GROUPS):
                print("%s %-12s %3d rows, largest bound / largest component %.2e" % (bound, name, (FIX["group"] == g).sum(), rel[FIX["group"] == g].max()))
            assert np.all(rel <= 1e-11)
        # chart change: informative rows (every compared component's bound <= 1e-10 max(1, |value|)) outside the planar group
        out = FIX["cc_group"] != PLANAR
        for name, val, B in (("1->2", FIX["cc_val12"], FIX["cc_B12"]), ("2->1", FIX["cc_val21"], FIX["cc_B21"])):
            inf = informative(val, B)
            for g, gname in enumerate(CC_GROUPS):
                sel = FIX["cc_group"] == g
                print("chart change %s %-14s informative %2d of %2d, largest bound / max(1, |value|) %.2e"
                      % (name, gname, inf[sel].sum(), sel.sum(), (B / np.maximum(1.0, np.abs(val)))[sel].max()))
            print("chart change %s: informative outside the planar group %.1f %%" % (name, 100 * inf[out].mean()))
            assert inf[out].mean() >= 0.9
            assert np.all(np.isfinite(B)) and np.all(np.isfinite(val))
    # the segments: a chart decision never closer than 1e-6 to the limit is the generator's assertion; here what they cover
    ch = FIX["seg_charts"]
    assert set(ch[0]) == {0, 1} and 0 not in ch[1] and list(ch[2][:2]) == [1, 2] and list(ch[3][:3]) == [1, 1, 1] and 2 in ch[3]


# ---- Part B: the reference and the emulations within the bounds ---------------------------------------------------------------

def with_alternatives(r, got, key, bound):
    r = r.copy()
    und = FIX["und"]
    r[und] = np.minimum(r[und], ratios(got[und], FIX["alt_" + key], FIX["alt_" + bound]))
    return r


def test_reference_within_b_ref(capsys):
    r = ratios(FIX["ref64_rhs"], FIX["val"], FIX["Bref"])
    ru = ratios(FIX["ref64_u"], FIX["u"], FIX["Bu"])
    rh = ratios(FIX["ref64_H"], FIX["H"], FIX["BH"])
    dec = FIX["dec"]
    with capsys.disabled():
        print()
        report("reference/B_ref", FIX["group"][dec], GROUPS, r[dec])
        report("reference control/B_u", FIX["group"][dec], GROUPS, ru[dec])
        report("reference H/B_H", FIX["group"][dec], GROUPS, rh[dec][:, None])
    assert np.all(with_alternatives(r, FIX["ref64_rhs"], "val", "Bref") <= 1.0)
    assert np.all(with_alternatives(ru, FIX["ref64_u"], "u", "Bu") <= 1.0)
    assert np.all(with_alternatives(rh, FIX["ref64_H"], "H", "BH") <= 1.0)
    assert np.all(r[dec] <= 1.0) and np.all(ru[dec] <= 1.0) and np.all(rh[dec] <= 1.0)


def chart_ratios(got, direction):
    """|got - value| / B of the chart rows; on an undecidable row the smaller of the two adjacent branches."""
    r = ratios(got, FIX["cc_val" + direction], FIX["cc_B" + direction])
    und = FIX["cc_und" + direction]
    r[und] = np.minimum(r[und], ratios(got[und], FIX["alt_cc_val" + direction], FIX["alt_cc_B" + direction]))
    return r


def test_reference_chart_changes_within_bound(capsys):
    """Every row, the undecidable ones on one of their two branches.  A flipped pivot is the same linear system eliminated in the
    other order: the same value to 240 bits, that order's bound."""
    r12, r21 = chart_ratios(FIX["ref64_c12"], "12"), chart_ratios(FIX["ref64_c21"], "21")
    with capsys.disabled():
        print()
        report("reference 1->2 / B", FIX["cc_group"], CC_GROUPS, r12)
        report("reference 2->1 / B", FIX["cc_group"], CC_GROUPS, r21)
    assert np.all(r12 <= 1.0) and np.all(r21 <= 1.0)
    tie12 = [i for i, n in zip(FIX["cc_und12"], FIX["cc_und12_names"]) if str(n) == "pivot0"]
    for k, i in enumerate(FIX["cc_und12"]):
        if i in tie12:
            assert np.all(np.abs(FIX["alt_cc_val12"][k] - FIX["cc_val12"][i]) <= 2.0 ** -52 * np.abs(FIX["cc_val12"][i]))


def test_float64_chart_change_on_either_pivot_within_its_bound():
    """The flipped-pivot path of the restatement in float64: taking the runner-up on the tie rows stays within the alternative's
    bound, taking the first largest within the stored one."""
    P = FIX["blocks"][int(FIX["cc_block"])]
    for k, i in enumerate(FIX["cc_und12"]):
        x = FIX["cc_X"][i]
        first = ir.emulate_chart(P, True, x)
        other = ir.emulate_chart(P, True, x, flip=("pivot0",))
        assert np.all(ratios(first, FIX["cc_val12"][i], FIX["cc_B12"][i]) <= 1.0)
        assert np.all(ratios(other, FIX["alt_cc_val12"][k], FIX["alt_cc_B12"][k]) <= 1.0)
        assert not np.array_equal(first, other)


@functools.lru_cache(maxsize=None)
def emulation(form, **kit):
    d, u, H = np.empty((N, 12)), np.empty((N, 2)), np.empty(N)
    for i in range(N):
        d[i], u[i], H[i] = ir.emulate_rhs(form, *row(i), **kit)
    return d, u, H


def test_float64_emulation_of_the_throughput_form_within_b_fast(capsys):
    d, u, H = emulation("fast")
    dec = FIX["dec"]
    r = ratios(d, FIX["val"], FIX["Bfast"])
    with capsys.disabled():
        print()
        report("float64/B_fast", FIX["group"][dec], GROUPS, r[dec])
    assert np.all(r[dec] <= 1.0), np.argwhere(r[dec] > 1.0)[:5]
    assert np.all(with_alternatives(r, d, "val", "Bfast") <= 1.0)
    assert np.all(np.isfinite(d))


def test_throughput_form_without_the_range_guard_fails_on_large_costates():
    """The defect the costate group found: rhs_fast squared |p_a1 c1| and |p_a2| into b2, which overflows from ~1e154 on, rsqrt(inf)
    is 0, and cos(beta) = sin(beta) = 0 drops the whole control term -- errors of 3e14 bounds.  Small costates (b2 underflowing to 0:
    cos(beta) = 1, sin(beta) = 0) stay within the bound because every term they enter is itself of the costates' size.  No earlier
    test fed such a state.  The emulation without the guard shows both; with it, test_float64_emulation_... passes."""
    d, _, _ = emulation("fast", no_b2_guard=True)
    r = ratios(d, FIX["val"], FIX["Bfast"])
    big = np.maximum(np.abs(FIX["X"][:, 8]), np.abs(FIX["X"][:, 9])) >= 1e155
    assert big.sum() >= 12 and np.all(r[big].max(axis=1) > 1e6)
    assert np.all(r[~big & FIX["dec"]] <= 1.0)


@pytest.mark.skipif(not fr.HAVE_MPMATH, reason="the generator's arithmetic (mpmath) is not installed")
def test_sample_rows_regenerate_bit_for_bit():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_interceptor_pin_golden as gen
    idx = np.unique(np.linspace(0, N - 1, gen.REGEN_ROWS).astype(int))
    for stored, fresh in gen.regenerate(FIX, idx):
        assert np.array_equal(np.asarray(stored), np.asarray(fresh, dtype=np.asarray(stored).dtype))
    P = FIX["blocks"][int(FIX["cc_block"])]
    for i in (0, NCC // 2, NCC - 1):
        e = ir.evaluate_chart(P, True, FIX["cc_X"][i])
        assert np.array_equal(e["value"], FIX["cc_val12"][i]) and np.array_equal(gen.round_up(e["B"]), FIX["cc_B12"][i])


# ---- Part B: wrong emulations -------------------------------------------------------------------------------------------------

def old_bar_rhs(d):
    """tests/test_gpu_interceptor.py's bar on a right-hand side, against the oracle (= the reference's doubles): the largest
    |f - fo| / max(1e-6 max|fo|, |fo|) over the nominal group; it passes below 1e-9."""
    nom = FIX["group"] == GROUPS.index("nominal")
    fo = FIX["ref64_rhs"][nom]
    return float(np.max(np.abs(d[nom] - fo) / np.maximum(1e-6 * np.abs(fo).max(axis=1, keepdims=True), np.abs(fo))))


def old_bar_chart(got, want):
    """rel() of tests/test_gpu_interceptor.py through a chart change; it passes below 1e-9."""
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


RHS_MUTATIONS = {
    "tan^2 theta dropped from chart 2's Xdot[8]": "tan2_dropped",
    "chart 2's sin(beta) without the sign of -p_phi": "sb_unsigned",
    "coasting mass computed with t instead of t1": "coast_mass_t",
    "second part of pi/2 left out of the short sincos": "pio2_tail_dropped",
}
BELOW_THE_OLD_BAR = ["second part of pi/2 left out of the short sincos"]


@pytest.mark.parametrize("name", list(RHS_MUTATIONS))
def test_mutations_of_the_right_hand_side_violate_b_fast(name, capsys):
    """Each wrong emulation leaves B_fast on a decidable row; the unmutated one on none.  Printed beside it: what the 1e-9 bar of
    tests/test_gpu_interceptor.py makes of the same emulation on the nominal group.  Asserted: that bar sees the dropped tan^2, the
    unsigned sin(beta) and the coasting mass as well (on generic states none of them is a small term), and does not see the truncated
    pi/2, which leaves the nominal rows' figure where the unmutated emulation has it and shows at the doubles nearest +-pi/2 and
    +-pi, where a sine or cosine of 6e-17 comes out as 0."""
    good, bad = emulation("fast")[0], emulation("fast", mutation=RHS_MUTATIONS[name])[0]
    dec = FIX["dec"]
    r = ratios(bad, FIX["val"], FIX["Bfast"])[dec]
    with capsys.disabled():
        print("\n%s: rows beyond B_fast %d of %d, largest err/B %.3g; old bar on the nominal group %.3e (unmutated %.3e)"
              % (name, (r > 1.0).any(axis=1).sum(), dec.sum(), r.max(), old_bar_rhs(bad), old_bar_rhs(good)))
    assert np.all(ratios(good, FIX["val"], FIX["Bfast"])[dec] <= 1.0)
    assert np.any(r > 1.0)
    assert (old_bar_rhs(bad) < 1e-9) == (name in BELOW_THE_OLD_BAR)


def test_mutation_of_jac_chart2_violates_the_chart_bound(capsys):
    """Two entries of jac_chart2 exchanged ((4,4) and (4,5)): beyond the bound on every row, and far beyond the old 1e-9 bar too."""
    P = FIX["blocks"][int(FIX["cc_block"])]
    good = np.array([ir.emulate_chart(P, True, x) for x in FIX["cc_X"]])
    bad = np.array([ir.emulate_chart(P, True, x, mutation="jac2_swap") for x in FIX["cc_X"]])
    r = ratios(bad, FIX["cc_val12"], FIX["cc_B12"])
    with capsys.disabled():
        print("\njac_chart2 entries exchanged: rows beyond the bound %d of %d; old bar %.3e (unmutated %.3e)"
              % ((r > 1.0).any(axis=1).sum(), NCC, old_bar_chart(bad, FIX["ref64_c12"]), old_bar_chart(good, FIX["ref64_c12"])))
    assert np.all(ratios(good, FIX["cc_val12"], FIX["cc_B12"]) <= 1.0)
    assert (r > 1.0).any(axis=1).sum() >= 0.9 * NCC and old_bar_chart(bad, FIX["ref64_c12"]) > 1e-9


def test_mutation_hand_back_skipped_violates_the_round_trip_bound():
    """A trajectory that ends in chart 2 and is not handed back: the zero-length round trip returns the chart-2 row."""
    P = FIX["blocks"][int(FIX["cc_block"])]
    for i in (0, 5, 20, 30):
        x = FIX["cc_X"][i]
        good, _ = ir.emulate_traj(P, 1, 0.0, 0.0, x)
        bad, _ = ir.emulate_traj(P, 1, 0.0, 0.0, x, mutation="no_handback")
        back = ir.emulate_chart(P, False, FIX["ref64_c12"][i])
        assert np.all(ratios(back, FIX["cc_val21"][i], FIX["cc_B21"][i]) <= 1.0)
        assert np.max(np.abs(good - back) / np.maximum(1.0, np.abs(back))) < 1e-9
        assert np.any(ratios(bad, FIX["cc_val21"][i], FIX["cc_B21"][i]) > 1.0) and old_bar_chart(bad, back) > 1e-9


def test_segments_float64_recurrence_within_the_allowance(capsys):
    """The yardstick of the GPU test, applied to the float64 restatements: 8x the pinned oracle's own deviation from the mpf
    trajectory per component, plus 8 u |X|."""
    U = 2.0 ** -53
    allowed = 8 * FIX["seg_dev"][None, :] + 8 * U * np.abs(FIX["seg_mpf"])
    for form in ("ref", "fast"):
        got = np.array([ir.emulate_traj(FIX["blocks"][0], int(FIX["seg_N"]), a, e, x, form)[0]
                        for a, e, x in zip(FIX["seg_t0"], FIX["seg_tf"], FIX["seg_X0"])])
        err = np.abs(got - FIX["seg_mpf"])
        with capsys.disabled():
            print("\nsegments, float64 %s form: err/allowed per component %s" % (form, " ".join("%.3f" % v for v in (err / allowed).max(axis=0))))
        assert np.all(err <= allowed)
    assert np.all(np.abs(FIX["ref64_seg"] - FIX["seg_mpf"]) <= FIX["seg_dev"][None, :] + 2 * U * np.abs(FIX["seg_mpf"]))      # seg_mpf is rounded
