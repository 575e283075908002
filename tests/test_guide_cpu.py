"""CPU: the definition of socp_guide_batch as tests/guide_reference.py restates it, on the polished roots and with the tables of
test_gain_cpu.py (every time FIXED: nominal Goddard at mu2 = 1 and 0.2, the double integrator; M = 1, N = 50) and of
test_gain_free_cpu.py (final time FREE: Goddard M = 1, the double integrator, Goddard M = 3 with N = 10).
(1) zero deviation is the nominal flight, bit for bit, in doubles (M = 1, and segment 0 of M = 3: across a node the flight goes on from
    its own state, so later segments carry the row's own continuity defect);
(2) meaning, in 240 bits: the miss of a flight corrected at every sample falls at second order with the deviation, the open-loop one
    at first order -- the bars of test_gain_cpu.py::test_2 and test_gain_free_cpu.py::test_2;
(3) the instrument: wrong restatements are caught by the measure of (2), the right one passes it;
(4) `every` and skipped samples, in doubles;
(5) the symbols and the launch table.  No GPU; the library is only asked for its symbols.

Measured (profiles/guide_cpu_tests.txt): see the lines of the run on record there."""
import os

import numpy as np
import pytest

import exact_jacobian_reference as ej
import fields_reference as fr
import guide_reference as gd
import test_gain_cpu as tg
import test_gain_free_cpu as tgf

pytestmark = pytest.mark.skipif(not fr.HAVE_MPMATH, reason="mpmath is the 240-bit carrier")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mpf = fr.mpf
_TAB = {}
FIXED_CASES = ("goddard", "goddard_mu02", "dint")
FREE_CASES = ("goddard", "dint", "goddard_m3")
ALL_CASES = [("fixed", n) for n in FIXED_CASES] + [("free", n) for n in FREE_CASES]
# (3): the measure of (2) is the pair (closed-loop miss per halving of the deviation, closed-loop miss as a fraction of the open-loop
# one).  A wrong restatement leaves a miss of FIRST order in the deviation (or one that does not depend on it at all): it halves (or
# stays) where the right one quarters.  The wrong ones are asked for a ratio below 2.5, halfway between first and second order, or a
# miss that is not finite; the right one for the bars of (2): a ratio of at least 3 and a fraction below 1e-4.  The fraction of every
# wrong one is recorded beside its ratio: K_p is the Hessian of the value function and symmetric up to the integrator's own
# departure from symplecticity, so reading it transposed leaves a FIRST-order miss of only 1e-8 of the open-loop one -- the ratio
# catches it, a fraction could not.
WRONG_RATIO = 2.5
RIGHT_BAR = 1e-4


def record(key, line):
    """The figures of a run (pytest -s): profiles/guide_cpu_tests.txt keeps the lines of the run on record."""
    print("[guide_cpu %s] %s" % (key, line))


def setup(kind, name):
    """(case, N, stride): the polished root of the gain tests."""
    if kind == "fixed":
        return tg.case(name), tg.N, 7
    c = tgf.case(name)
    return c, c["N"], c["stride"]


def tables(kind, name, high):
    """The tables of the row, from the gain tests' own (cached) restatement rows."""
    key = (kind, name, high)
    if key not in _TAB:
        c, N, stride = setup(kind, name)
        segs = [tg.rows(name, stride, high)] if kind == "fixed" else tgf.rows(name, stride, high)
        _TAB[key] = gd.tables_of(segs, kind == "free")
    return _TAB[key]


def fly(kind, name, dx0, every, high=False, mutate=(), tab=None, stop_at=None):
    c, N, stride = setup(kind, name)
    tab = tables(kind, name, high) if tab is None else tab
    return gd.guide_case(c["model"], c["P"], c["sw"], c["prob"], c["z"], N, stride, tab, dx0, every, high=high, mutate=mutate, stop_at=stop_at)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- (1) zero deviation is the nominal flight -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,name", ALL_CASES)
def test_1_zero_deviation_is_the_nominal_flight(kind, name):
    c, N, stride = setup(kind, name)
    prob, D = c["prob"], c["D"]
    M, n = prob.M, len(c["z"])
    tab = tables(kind, name, False)
    r = fly(kind, name, [0.0] * D, 1)
    samples = sum(t["count"] for t in tab)
    _, F = ej.exact_jacobian_row(c["model"], c["P"], c["sw"], prob, c["z"], N, derivs=False)
    want = [F[D + j] for j in range(D)]
    if kind == "free":
        want.append(F[ej.Layout(prob).ft_row[M]])
    for i in range(M):
        assert len(r["xs"][i]) == tab[i]["count"]
    for q in range(tab[0]["count"]):
        assert np.array_equal(bits(r["xs"][0][q]), bits(tab[0]["xq"][q])), "Xs equals the table's Xq bit for bit (segment 0 sample %d)" % q
    tf_nom = float(c["z"][n - 1] if kind == "free" else prob.time[M])
    if M == 1:
        assert bits([r["tf"]])[0] == bits([tf_nom])[0]
        assert np.array_equal(bits(r["miss"]), bits(want)), "miss equals the residual's final rows"
        assert r["dxmax"] == 0.0
    else:
        # the flight goes on from ITS OWN state across a node, the table's samples of a later segment start from the node's unknowns:
        # the two differ by the row's own continuity defect, which the residual reports.  Exact: the state part of the first sample
        # of segment 1 is off by the residual's continuity rows of node 1, bit for bit (the same subtraction on the same numbers).
        # Everything after it is a linear image of the two nodes' defects under the closed loop, whose transition over a third of this
        # 0.26 s flight has a norm of order ten (the blocks Psi of the table): asked to stay within 1e2 of the residual's norm and of the
        # rounding of the unknowns (the figure is recorded)
        S = 2 * D
        x1 = [r["xs"][1][0][j] - tab[1]["xq"][0][j] for j in range(D)]
        assert np.array_equal(bits(x1), bits([F[S + j] for j in range(D)])), "the first sample of segment 1 is off by the residual's continuity rows"
        room = 1e2 * (float(np.abs(F).max()) + 2.0 ** -52 * float(np.abs(c["z"]).max()))
        worst = max(abs(a - b) for i in range(1, M) for q in range(tab[i]["count"]) for a, b in zip(r["xs"][i][q], tab[i]["xq"][q]))
        worst_m = max(abs(a - b) for a, b in zip(r["miss"], want))
        record("1 %s %s" % (kind, name), "M = %d: later segments off Xq by at most %.3e, miss off the residual's rows by %.3e (room %.3e, ||F||inf = %.3e)"
               % (M, worst, worst_m, room, float(np.abs(F).max())))
        assert worst <= room and worst_m <= room and r["dxmax"] <= room and abs(r["tf"] - tf_nom) <= room
    assert r["nupd"] + r["nskip"] == samples == r["samples"]
    record("1 %s %s" % (kind, name), "dX0 = 0, every = 1: %d samples (%d corrected, %d skipped), Xs = Xq and miss = the residual's final rows bit for bit; "
           "||miss||inf = %.3e" % (samples, r["nupd"], r["nskip"], max(abs(float(v)) for v in r["miss"])))


# ---- (2) the meaning, in 240 bits ---------------------------------------------------------------------------------------------------------

def measure(kind, name, j, every, half, mutate=(), scale=mpf("1e-9")):
    """||miss(delta e_j) - miss(0)||inf of a flight in 240 bits; delta = scale max(1, |x_j|) / 2^half.  A NaN miss counts as infinite."""
    c, N, stride = setup(kind, name)
    D = c["D"]
    x = mpf(float(c["z"][j]))
    dx0 = [mpf(0)] * D
    dx0[j] = scale * max(mpf(1), abs(x)) / (2 ** half)
    base = fly(kind, name, [mpf(0)] * D, every, high=True)["miss"]
    got = fly(kind, name, dx0, every, high=True, mutate=mutate)["miss"]
    if any(v != v for v in got):
        return mpf("inf")
    return max(abs(a - b) for a, b in zip(got, base))


@pytest.mark.parametrize("kind,name", ALL_CASES)
def test_2_closed_loop_miss_is_second_order(kind, name):
    """delta = 1e-9 max(1, |x_j|) at the first sample, then half of it, j = 0 and d - 1: with every = 1 the miss (the H row included when
    the final time is FREE) falls by >= 3 per halving or is zero to 240-bit rounding (the linear double integrator), with every = 0 by
    1.8 .. 2.2, and the closed-loop miss is below 1e-4 of the open-loop one."""
    c, N, stride = setup(kind, name)
    D = c["D"]
    ok = True
    with fr.mpmath.workprec(240):
        for j in (0, D - 1):
            m = {(e, h): measure(kind, name, j, e, h) for e in (1, 0) for h in (0, 1)}
            rc = m[1, 0] / m[1, 1] if m[1, 1] != 0 else mpf("inf")
            ru = m[0, 0] / m[0, 1]
            linear = m[1, 0] <= tg.TOL_CHAIN * m[0, 0] and m[1, 1] <= tg.TOL_CHAIN * m[0, 1]
            ok = ok and (linear or rc >= 3) and mpf("1.8") <= ru <= mpf("2.2") and m[1, 0] < m[0, 0] * mpf("1e-4")
            record("2 %s %s" % (kind, name), "x_%d: every = 1 miss %.3e -> %.3e (ratio %.3f), every = 0 miss %.3e -> %.3e (ratio %.3f), closed / open %.3e"
                   % (j, float(m[1, 0]), float(m[1, 1]), float(rc), float(m[0, 0]), float(m[0, 1]), float(ru), float(m[1, 0] / m[0, 0])))
            # a report, not asserted: a large deviation, corrected at every sample, at every fifth, once
            big = {e: measure(kind, name, j, e, 0, scale=mpf("1e-3")) for e in (1, 5, 10 ** 6, 0)}
            record("2 %s %s" % (kind, name), "x_%d, delta = 1e-3 max(1, |x|): miss with every = 1 %.3e, every = 5 %.3e, once %.3e, open loop %.3e"
                   % (j, float(big[1]), float(big[5]), float(big[10 ** 6]), float(big[0])))
    assert ok, "the closed-loop miss falls by at least 3 per halving (or is zero to rounding), the open-loop one by about 2"


# ---- (3) the instrument ---------------------------------------------------------------------------------------------------------------------

MUTATION_CASES = {"no_retime": ("free", "goddard"), "clock_restart": ("free", "goddard")}


def ratio_and_fraction(kind, name, mutate):
    """The measure of (2) at j = 0 and j = d - 1: (the smaller miss ratio per halving, the larger fraction of the open-loop miss)."""
    D = setup(kind, name)[0]["D"]
    ratios, fractions = [], []
    for j in (0, D - 1):
        m0, m1 = measure(kind, name, j, 1, 0, mutate=mutate), measure(kind, name, j, 1, 1, mutate=mutate)
        ratios.append(m0 / m1 if mpf("-inf") < m0 < mpf("inf") and 0 < m1 < mpf("inf") else mpf("nan"))
        fractions.append(m0 / measure(kind, name, j, 0, 0))
    return ratios, max(fractions)


@pytest.mark.parametrize("mutation", gd.MUTATIONS)
def test_3_wrong_restatements_are_caught(mutation):
    kind, name = MUTATION_CASES.get(mutation, ("fixed", "goddard"))
    with fr.mpmath.workprec(240):
        ratios, f = ratio_and_fraction(kind, name, (mutation,))
    record("3 " + mutation, "wrong restatement %-15s on %s %s: closed-loop miss ratio per halving %s (bar < %.1f or not finite), %.3e of the open-loop miss"
           % (mutation, kind, name, ", ".join("%.3f" % float(r) for r in ratios), WRONG_RATIO, float(f)))
    assert any(r != r or r < WRONG_RATIO for r in ratios), "a wrong restatement leaves a first-order miss"


def test_3_the_right_restatement_passes_the_same_measure():
    with fr.mpmath.workprec(240):
        for kind, name in (("fixed", "goddard"), ("free", "goddard")):
            ratios, f = ratio_and_fraction(kind, name, ())
            record("3 none", "the right restatement on %s %s: ratio per halving %s (bar >= 3), %.3e of the open-loop miss (bar < %.0e)"
                   % (kind, name, ", ".join("%.3f" % float(r) for r in ratios), float(f), RIGHT_BAR))
            assert all(r >= 3 for r in ratios) and f < RIGHT_BAR


# ---- (4) `every` and skipped samples -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,name", [("fixed", "goddard"), ("free", "goddard_m3")])
def test_4_every_and_skipped_samples(kind, name):
    c, N, stride = setup(kind, name)
    D = c["D"]
    tab = tables(kind, name, False)
    samples = sum(t["count"] for t in tab)
    dx0 = [1e-6 * max(1.0, abs(float(c["z"][j]))) for j in range(D)]
    runs = {e: fly(kind, name, dx0, e) for e in (0, 1, 3, samples + 5)}
    assert (runs[0]["nupd"], runs[0]["nskip"], runs[0]["dxmax"]) == (0, 0, 0.0), "every = 0 is the open-loop flight"
    assert runs[1]["nupd"] + runs[1]["nskip"] == samples
    assert runs[3]["nupd"] + runs[3]["nskip"] == -(-samples // 3)
    assert (runs[samples + 5]["nupd"], runs[samples + 5]["nskip"]) == (1, 0), "a very large `every` corrects once, at the first sample"
    off_tail = sum(1 for t in tab for v in t["info"] if v != 0)
    assert runs[1]["nskip"] == off_tail
    if kind == "fixed":
        assert off_tail > 0, "the thrust-off tail of the nominal Goddard flight has no gain"
    assert not np.array_equal(bits(runs[1]["xf"]), bits(runs[0]["xf"])) and not np.array_equal(bits(runs[1]["xf"]), bits(runs[3]["xf"]))
    # info forced to 1 from sample g0 on: the costate left flowing from that sample
    g0 = 2
    forced, g = [], 0
    for t in tab:
        info = [v if g + q < g0 else 1 for q, v in enumerate(t["info"])]
        g += t["count"]
        forced.append(dict(t, info=info))
    a, b = fly(kind, name, dx0, 1, tab=forced), fly(kind, name, dx0, 1, stop_at=g0)
    assert np.array_equal(bits(a["xf"]), bits(b["xf"])) and np.array_equal(bits(a["miss"]), bits(b["miss"]))
    assert (a["nupd"], a["nskip"]) == (g0, samples - g0) == (b["nupd"], b["nskip"])
    assert not np.array_equal(bits(a["xf"]), bits(runs[1]["xf"]))
    # the same cut-off read by the wrong restatement that ignores info: it applies the (finite) gains the caller disabled, and shows
    wrong = fly(kind, name, dx0, 1, tab=forced, mutate=("ignore_info",))
    assert wrong["nupd"] > g0 and not np.array_equal(bits(wrong["xf"]), bits(a["xf"])), "ignoring info on a real table changes the flight"
    record("4 %s %s" % (kind, name), "%d samples, %d without a gain: every = 0 / 1 / 3 / %d corrects %d / %d / %d / %d times; ||miss||inf %.3e / %.3e / %.3e / %.3e; "
           "cut off after %d samples: %.3e" % (samples, off_tail, samples + 5, runs[0]["nupd"], runs[1]["nupd"], runs[3]["nupd"], runs[samples + 5]["nupd"],
                                              *[max(abs(v) for v in runs[e]["miss"]) for e in (0, 1, 3, samples + 5)], g0, max(abs(v) for v in a["miss"])))


# ---- (5) the symbols ----------------------------------------------------------------------------------------------------------------------------

def test_5_symbols_and_launch_table():
    from socp_amd import capi
    L = capi.lib()
    for sym in ("socp_ctx_has_guide", "socp_guide_batch_dev", "socp_guide_batch", "socp_guide_batch_blocks"):
        assert hasattr(L, sym), sym
    for method in ("guide_batch", "guide_batch_dev", "has_guide"):
        assert hasattr(capi.Context, method), method
    src = lambda *p: open(os.path.join(ROOT, *p)).read()                                           # noqa: E731
    launch = src("socp_amd", "csrc", "launch.hpp")
    assert "kPluginAbi = 20;" in launch and "(*guide)" in launch
    make = src("socp_amd", "csrc", "Makefile")
    assert "kernels_guide.o" in make and "kernels_guide_fast.o" in make
    # the four in-tree instantiations, in both flavours' objects, each table pointing to its own flavour's launcher
    exact, fast = src("socp_amd", "csrc", "kernels_guide.hip"), src("socp_amd", "csrc", "kernels_guide_fast.hip")
    for m in ("GoddardExactSmooth", "GoddardExact", "DIntExact", "CovidExact"):
        assert "plugin::guide<%s>" % m in exact, m
    for m in ("GoddardFastSmooth", "GoddardFast", "CovidFast"):
        assert "plugin::guide<%s>" % m in fast, m
    assert "plugin::guide<DInt" not in fast, "the double integrator is one struct in both flavours: one instantiation, in kernels_guide.hip"
    tables_ = src("socp_amd", "csrc", "builtin_tables.hpp")
    for m in ("goddard", "covid"):
        assert "t.guide = kRef ? &guide_%s : &guide_%s_fast;" % (m, m) in tables_
    assert "t.guide = &guide_dint;" in tables_
    # absent for the interceptor, vtolUAV and lqr1d: the trait excludes the hooks they bring
    impl = src("socp_amd", "csrc", "plugin_impl.hpp")
    assert "struct has_guide : std::bool_constant<!has_custom_traj<M>::value && !has_custom_final<M>::value && !has_switching_state<M>::value>" in impl
    assert "kCustomTraj = true" in src("socp_amd", "csrc", "models_interceptor.hpp")
    assert "kCustomFinal = true" in src("socp_amd", "csrc", "models_vtol.hpp")
    assert "switching_state(" in src("tests", "plugin", "lqr1d_plugin.hip")
