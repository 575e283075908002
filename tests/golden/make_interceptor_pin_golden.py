#!/usr/bin/env python3
"""Writes tests/golden/interceptor_pin.npz: the rows that pin the interceptor (read by tests/test_interceptor_pin_cpu.py and
tests/test_gpu_interceptor_pin.py).  Two kinds of numbers, data only:

  ref64_* / a_*   the REFERENCE's own doubles: its interceptor.cpp compiled as it lies against oracle/eigen_shim
                  (oracle/_ref/libsocp_ref_interceptor.so, built by `make -C oracle ref`), asked through oracle.RefInterceptor;
  val, B*, ...    the 240-bit values and derived bounds of tests/interceptor_reference.py.

Authoring machine only: needs mpmath and the reference build.  Tests read the file and never the reference.

    python tests/golden/make_interceptor_pin_golden.py [out.npz]

Layout.  blocks[nb, 18]: parameter blocks (slot order of include/socp_hip.h).  Right-hand-side rows: group (index into group_names),
block, chart, stage, t, X[12]; val[12], Bref[12], Bfast[12], u[2] = (u, beta), Bu[2], H, BH; dec; und and alt_* (the same on the
other side of the undecided decisions), und_names; ref64_rhs, ref64_u, ref64_H.  Chart-change rows: cc_group (index into cc_group_names), cc_X;
cc_val12, cc_B12, cc_dec12: ConversionState12 of cc_X, with cc_und12, cc_und12_names and alt_cc_val12, alt_cc_B12 (the other side of
the undecided decisions: for a pivot tie the same value by the other elimination order, with that order's bound); ref64_c12, ref64_c21 (the reference's ConversionState21 of ITS chart-2 row) and
cc_val21, cc_B21, cc_dec21 (cc_und21, cc_und21_names, alt_cc_val21, alt_cc_B21): the 240-bit ConversionState21 of ref64_c12 taken as exact doubles.  Segments: seg_t0, seg_tf, seg_X0,
seg_N, seg_mpf (the same recurrence in mpf, chart decisions on exact values), seg_charts (the chart of every stored row), seg_dev (the
reference-order CPU oracle's deviation from seg_mpf per component, maximum over the starts), ref64_seg.  Part A only (a_*): whole
trajectories with flags, final rows, the analytical guess.  Bounds are rounded UP to 12 significant bits."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import fast_reference as fr                                   # noqa: E402
import interceptor_reference as ir                            # noqa: E402
from oracle.oracle import Oracle, RefInterceptor, have_ref_interceptor, MODEL_INTERCEPTOR   # noqa: E402

GROUPS = ["nominal", "near_limit", "angles", "control", "costates"]
CC_GROUPS = ["generic", "near_vertical", "vertical", "planar", "pivot_tie"]
BOUND_BITS = 12
R_E = 6378145.0
T1 = 20.0                                                     # propellant_mass / q of every block used
STAGE_T = [(1, 3.0), (1, T1), (0, T1), (0, 27.0)]
SEG_N = 5
ISOLATION_LIMIT = 2.0                                         # chartLimit of the chart-change-in-isolation block: every state changes
REGEN_ROWS = 10
HALF_PI, PI = np.pi / 2.0, float(np.pi)


def block(**kw):
    p = ir.SHIPPED.copy()
    names = ["c0", "hr", "d0", "eta", "propellant_mass", "empty_mass", "q", "ve", "alpha_max", "u_max", "a_max", "mu_gft", "muT", "muV",
             "muC", "R_Earth", "mu0", "chartLimit"]
    for k, v in kw.items():
        p[names.index(k)] = v
    return p


BLOCKS = [block(), block(mu_gft=0.6, muC=0.05), block(chartLimit=ISOLATION_LIMIT)]


def scenario_state(o, gamma=np.pi / 4, chi=0.0):
    """The test program's initial state with the analytical costate guess (as tests/test_gpu_interceptor.py builds it)."""
    Xi = np.zeros(12)
    Xi[:6] = [1000, 1000, gamma, chi, 5454661 / R_E, 46086 / R_E]
    Xf = np.zeros(12)
    Xf[:6] = [6000, 1000, 0.01 * np.pi, 0.01 * np.pi, (5454661 + 27829.0) / R_E, 46086 / R_E]
    return o.init_analytical(0.0, Xi, 10.0, Xf), Xf


def spread_states(o, B, seed=3):
    """states_both_charts of tests/test_gpu_interceptor.py: (chart-1 rows, the same states in chart 2)."""
    rng = np.random.default_rng(seed)
    X1, _ = scenario_state(o)
    rows1, rows2 = [], []
    for _ in range(B):
        x = X1 * (1 + 0.2 * rng.uniform(-1, 1, 12))
        x[2] = rng.uniform(-1.3, 1.3)
        x[3] = rng.uniform(-3, 3)
        rows1.append(x)
        rows2.append(o.chart12(x))
    return np.array(rows1), np.array(rows2)


def u_of(o, b, chart, stage, t, x):
    """The unsaturated control of the row, in float64 (only used to place rows: the fixture's numbers do not come from here)."""
    P = BLOCKS[b].copy()
    P[ir.UMAX] = 1e300
    return float(ir.emulate_rhs("ref", P, chart, stage, t, x)[1][0])


def rows_all(o):
    rows = []

    def add(group, b, chart, stage, t, X):
        rows.append(dict(group=group, block=b, chart=chart, stage=stage, t=float(t), X=np.array(X, dtype=float)))

    X1, X2 = spread_states(o, 4)
    both = ((1, X1), (2, X2))
    for b in (0, 1):
        for chart, Xs in both:
            for stage, t in STAGE_T:
                for x in Xs:
                    add("nominal", b, chart, stage, t, x)
    for chart, Xs in both:                                    # the flags are inputs: the mass with either flag on either side of t1
        add("nominal", 0, chart, 1, 27.0, Xs[0])
        add("nominal", 0, chart, 0, 3.0, Xs[0])
    limit = BLOCKS[0][ir.CHART_LIMIT]
    for chart, Xs in both:
        for k, c in enumerate([limit * (1 + 1e-3), limit * (1 - 1e-3), 1e-2, 1e-3, 1e-6]):
            for sign in (1, -1):
                for stage, t in ((1, 3.0), (0, 27.0)):
                    x = Xs[k % len(Xs)].copy()
                    x[2] = sign * np.arccos(c)
                    add("near_limit", 0, chart, stage, t, x)
    for chart, Xs in both:
        for k, a2 in enumerate([3.0, -3.0, PI, -PI, HALF_PI, -HALF_PI, 100.0, -100.0, 1e4, -1e4]):
            assert abs(a2) <= ir.SINCOS_FAST_RANGE
            x = Xs[k % len(Xs)].copy()
            x[3] = a2
            add("angles", 0, chart, 1, 3.0, x)
        for a1 in (0.0, -0.0):
            x = Xs[1].copy()
            x[2] = a1
            add("angles", 0, chart, 1, 3.0, x)
        for L in (0.0, 1.2, -1.2):
            x = Xs[2].copy()
            x[4] = L
            add("angles", 0, chart, 1, 3.0, x)
    for chart, Xs in both:
        for stage, t in ((1, 3.0), (0, 27.0)):
            x0 = Xs[0].copy()
            u0 = u_of(o, 0, chart, stage, t, x0)
            for target in (0.5, -0.5, 2.0, -2.0, 1.0, -1.0, 1 + 1e-15, 1 - 1e-15, -1 - 1e-15, 1 + 1e-9, 1 - 1e-9):
                x = x0.copy()
                x[8:10] *= target / u0                        # beta is invariant under the scaling, u linear in it (muC = 0)
                add("control", 0, chart, stage, t, x)
            x = x0.copy()
            x[7] = 1e-12                                      # den small, u saturates
            add("control", 0, chart, stage, t, x)
            x = x0.copy()
            x[7] = 1e-9
            x[8:10] *= 1e-10                                  # den small, |u| below the saturation
            add("control", 0, chart, stage, t, x)
            x = x0.copy()
            x[8:10] = 0.0
            add("control", 0, chart, stage, t, x)
            for z in (0.0, -0.0):
                x = x0.copy()
                x[8] = -abs(x[8]) * np.sign(np.cos(x[2]))     # p_a1 c1 < 0
                x[9] = z
                add("control", 0, chart, stage, t, x)
    for chart, Xs in both:
        for k, m in enumerate([1e-140, 1e-150, 1e-160, 1e-170, 1e150, 1e155, 1e160]):
            for s1, s2 in ((1, 1), (-1, 1), (1, -1)):
                x = Xs[k % len(Xs)].copy()
                x[8], x[9] = s1 * m, s2 * 0.7 * m
                add("costates", 0, chart, 1, 3.0, x)
        for pa1, pa2 in ((1e160, 1e-170), (1e-170, 1e-100), (1e-100, 1e-170)):
            x = Xs[3].copy()
            x[8], x[9] = pa1, pa2
            add("costates", 0, chart, 1, 3.0, x)
    return rows


def chart_rows(o):
    rng = np.random.default_rng(20261019)
    X1, _ = scenario_state(o)
    rows = []

    def add(group, gamma, chi):
        x = X1 * (1 + 0.2 * rng.uniform(-1, 1, 12))
        x[2], x[3] = gamma, chi
        rows.append((group, x))

    for _ in range(28):
        add("generic", rng.uniform(-1.5, 1.5), rng.uniform(-3.1, 3.1))
    for c in (0.09, 0.05, 0.02, 1e-2):
        for sign in (1, -1):
            for _ in range(2):
                add("near_vertical", sign * np.arccos(c), rng.uniform(-3.1, 3.1))
    add("vertical", HALF_PI, 0.7)
    add("vertical", -HALF_PI, -2.1)
    for chi in (0.0, PI):
        for g in (0.3, -0.8, 1.5, -1.52):
            add("planar", g, chi)
    for _ in range(4):                                        # l == L: the first column of either Jacobian holds -r sin L cos l and
        add("pivot_tie", rng.uniform(-1.2, 1.2), rng.uniform(-3.0, 3.0))     # -r cos L sin l, equal in value: the first pivot is a tie
        rows[-1][1][5] = rows[-1][1][4]
    assert len(rows) <= 64
    return rows


def segments(o):
    X0, _ = scenario_state(o)
    Xs, _ = scenario_state(o, gamma=1.49)
    Xc, _ = scenario_state(o, gamma=1.3)
    return [(0.0, 2.0, X0), (18.0, 22.0, X0), (0.0, 2.0, Xs), (0.0, 2.0, Xc)]


def round_up(b):
    b = np.asarray(b, dtype=float)
    m, e = np.frexp(b)
    r = np.ldexp(np.ceil(m * 2.0 ** BOUND_BITS) / 2.0 ** BOUND_BITS, e)
    return np.where((b == 0) | (b < 2.0 ** -1000) | ~np.isfinite(b), b, r)


KEYS = [("val", "value"), ("Bref", "B_ref"), ("Bfast", "B_fast"), ("u", "u"), ("Bu", "B_u"), ("H", "H"), ("BH", "B_H")]


def stored(e, key, src):
    q = np.asarray(e[src])
    return round_up(q) if key.startswith("B") else q


def evaluate(r, flip=()):
    return ir.evaluate_row(BLOCKS[r["block"]], r["chart"], r["stage"], r["t"], r["X"], flip=flip)


def regenerate(fix, idx):
    """Rows idx of the stored fixture evaluated afresh: [(stored, fresh)] arrays to compare bit for bit."""
    pairs = []
    for i in idx:
        e = ir.evaluate_row(fix["blocks"][fix["block"][i]], int(fix["chart"][i]), int(fix["stage"][i]), float(fix["t"][i]), fix["X"][i])
        for key, src in KEYS:
            pairs.append((fix[key][i], stored(e, key, src)))
        pairs.append((np.array(fix["dec"][i]), np.array(e["decidable"])))
    return pairs


def main(out_path):
    if not have_ref_interceptor():
        raise SystemExit("oracle/_ref/libsocp_ref_interceptor.so not built: make -C oracle ref")
    o = Oracle(MODEL_INTERCEPTOR)
    rows = rows_all(o)
    ev = [evaluate(r) for r in rows]
    keep = [i for i, e in enumerate(ev) if e["finite"]]
    print("rows %d, of which the 240-bit value is finite: %d" % (len(rows), len(keep)))
    rows, ev = [rows[i] for i in keep], [ev[i] for i in keep]
    out = {"group_names": np.array(GROUPS), "cc_group_names": np.array(CC_GROUPS), "blocks": np.array(BLOCKS),
           "group": np.array([GROUPS.index(r["group"]) for r in rows], dtype=np.int8),
           "block": np.array([r["block"] for r in rows], dtype=np.int8),
           "chart": np.array([r["chart"] for r in rows], dtype=np.int8),
           "stage": np.array([r["stage"] for r in rows], dtype=np.int8),
           "t": np.array([r["t"] for r in rows]), "X": np.array([r["X"] for r in rows])}
    for key, src in KEYS:
        out[key] = np.array([stored(e, key, src) for e in ev])
    out["dec"] = np.array([e["decidable"] for e in ev])
    und = [i for i, e in enumerate(ev) if not e["decidable"]]
    alt = [evaluate(rows[i], flip=ev[i]["undecided"]) for i in und]
    out["und"] = np.array(und, dtype=np.int32)
    out["und_names"] = np.array([";".join(ev[i]["undecided"]) for i in und])
    for key, src in KEYS:
        out["alt_" + key] = np.array([stored(e, key, src) for e in alt]).reshape((len(und),) + out[key].shape[1:])
    for g, name in enumerate(GROUPS):
        sel = out["group"] == g
        print("%-12s %4d rows, decidable %.1f %%; undecided: %s" % (name, sel.sum(), 100 * out["dec"][sel].mean(),
              sorted(set(n for i in np.flatnonzero(sel) for n in ev[i]["undecided"]))))
    assert len(und) and len(und) <= 0.1 * len(rows)

    # the reference's own doubles for the same rows
    refs = [RefInterceptor(params=b) for b in BLOCKS]
    R = np.empty((len(rows), 15))
    for i, r in enumerate(rows):
        ref = refs[r["block"]]
        ref.set_flags(r["chart"], r["stage"])
        R[i] = np.concatenate([ref.rhs(r["t"], r["X"]), ref.control(r["t"], r["X"]), ref.hamiltonian(r["t"], r["X"])])
    out["ref64_rhs"], out["ref64_u"], out["ref64_H"] = R[:, :12], R[:, 12:14], R[:, 14]

    # chart change in isolation
    cc = chart_rows(o)
    P = BLOCKS[2]
    out["cc_block"] = np.array(2)
    out["cc_group"] = np.array([CC_GROUPS.index(g) for g, _ in cc], dtype=np.int8)
    out["cc_X"] = np.array([x for _, x in cc])
    e12 = [ir.evaluate_chart(P, True, x) for _, x in cc]
    out["cc_val12"] = np.array([e["value"] for e in e12])
    out["cc_B12"] = np.array([round_up(e["B"]) for e in e12])
    out["cc_dec12"] = np.array([e["decidable"] for e in e12])
    und12 = [i for i, e in enumerate(e12) if not e["decidable"]]
    alt12 = [ir.evaluate_chart(P, True, cc[i][1], flip=e12[i]["undecided"]) for i in und12]
    out["cc_und12"] = np.array(und12, dtype=np.int32)
    out["cc_und12_names"] = np.array([";".join(e12[i]["undecided"]) for i in und12])
    out["alt_cc_val12"] = np.array([e["value"] for e in alt12]).reshape(len(und12), 12)
    out["alt_cc_B12"] = np.array([round_up(e["B"]) for e in alt12]).reshape(len(und12), 12)
    out["ref64_c12"] = np.array([refs[2].chart12(x) for _, x in cc])
    out["ref64_c21"] = np.array([refs[2].chart21(x) for x in out["ref64_c12"]])
    e21 = [ir.evaluate_chart(P, False, x) for x in out["ref64_c12"]]
    out["cc_val21"] = np.array([e["value"] for e in e21])
    out["cc_B21"] = np.array([round_up(e["B"]) for e in e21])
    out["cc_dec21"] = np.array([e["decidable"] for e in e21])
    out["cc_und21_names"] = np.array([";".join(e["undecided"]) for e in e21])
    und21 = [i for i, e in enumerate(e21) if not e["decidable"]]
    alt21 = [ir.evaluate_chart(P, False, out["ref64_c12"][i], flip=e21[i]["undecided"]) for i in und21]
    out["cc_und21"] = np.array(und21, dtype=np.int32)
    out["alt_cc_val21"] = np.array([e["value"] for e in alt21]).reshape(len(und21), 12)
    out["alt_cc_B21"] = np.array([round_up(e["B"]) for e in alt21]).reshape(len(und21), 12)
    assert any("pivot" in n for n in out["cc_und12_names"]) and any("pivot" in str(out["cc_und21_names"][i]) for i in und21)
    assert len(und12) <= 0.1 * len(cc) and len(und21) <= 0.1 * len(cc)
    for g, name in enumerate(CC_GROUPS):
        sel = out["cc_group"] == g
        print("chart change %-14s %3d rows, decidable 1->2 %d, 2->1 %d; undecided: %s" % (
            name, sel.sum(), out["cc_dec12"][sel].sum(), out["cc_dec21"][sel].sum(),
            sorted(set(n for i in np.flatnonzero(sel) for n in e12[i]["undecided"] + e21[i]["undecided"]))))

    # segments: the same recurrence in mpf, chart decisions on exact values with a margin of 1e-6 at least
    segs = segments(o)
    orc = Oracle(MODEL_INTERCEPTOR, step_nbr=SEG_N)
    ref5 = RefInterceptor(step_nbr=SEG_N)
    mp, charts, ref_seg, dev = [], [], [], []
    for a, e, x in segs:
        Xd, Xm, margin, flags = ir.traj_mpf(BLOCKS[0], SEG_N, a, e, x)
        assert margin >= 1e-6, (a, e, margin)
        got = orc.traj(a, x, e)
        assert np.array_equal(got, ref5.traj(a, x, e))
        mp.append(Xd)
        charts.append([c for c, _ in flags] + [0] * (2 * SEG_N + 3 - len(flags)))
        ref_seg.append(got)
        dev.append([fr._up(abs(fr.mpf(float(got[c])) - Xm[c])) for c in range(12)])
        print("segment %g -> %g: charts %s, smallest chart-limit margin %.3g" % (a, e, "".join(str(c) for c, _ in flags), margin))
    assert set(charts[0]) == {1, 0} and 0 not in charts[1] and charts[2][:2] == [1, 2] and charts[3][:3] == [1, 1, 1] and 2 in charts[3]
    out.update(seg_t0=np.array([s[0] for s in segs]), seg_tf=np.array([s[1] for s in segs]), seg_X0=np.array([s[2] for s in segs]),
               seg_N=np.array(SEG_N), seg_mpf=np.array(mp), seg_charts=np.array(charts, dtype=np.int8), ref64_seg=np.array(ref_seg),
               seg_dev=np.array(dev).max(axis=0))

    # Part A only: whole trajectories (50 steps per stage) with the flags they leave, final rows, the analytical guess
    ref = refs[0]
    X0, Xf = scenario_state(o)
    Xs, _ = scenario_state(o, gamma=1.49)
    Xn, _ = scenario_state(o, gamma=0.3)
    cases = [(0.0, 10.0, X0), (0.0, 30.0, X0), (22.0, 31.0, X0), (0.0, 6.0, Xs), (0.0, 25.0, Xs), (0.0, 1.0, Xn), (19.5, 20.5, Xn), (20.0, 21.0, Xn)]
    a_Xf, a_flags = [], []
    for a, e, x in cases:
        a_Xf.append(ref.traj(a, x, e))
        a_flags.append(ref.flags())
    print("whole trajectories end with (chart, stage): %s" % a_flags)
    assert {c for c, _ in a_flags} == {1, 2}
    out.update(a_traj_t0=np.array([c[0] for c in cases]), a_traj_tf=np.array([c[1] for c in cases]), a_traj_X0=np.array([c[2] for c in cases]),
               a_traj_Xf=np.array(a_Xf), a_traj_flags=np.array(a_flags, dtype=np.int8))
    fin_in, fin_out = [], []
    Xtf = a_Xf[1]
    for gammaf in (0.01 * np.pi, HALF_PI, -HALF_PI + 5e-6, HALF_PI - 2e-5):
        for mode in ([0, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1], [0, 0, 1, 0, 1, 0]):
            xd = Xf.copy()
            xd[2] = gammaf
            for chart, stage in ((1, 1), (2, 0)):
                ref.set_flags(chart, stage)
                fin_in.append(np.concatenate([[chart, stage, 30.0], mode, Xtf, xd]))
                fin_out.append(np.concatenate([ref.final_rows(0, 30.0, Xtf, xd, mode), ref.final_rows(1, 30.0, Xtf, xd, mode)]))
    out.update(a_final_in=np.array(fin_in), a_final_out=np.array(fin_out))
    rng = np.random.default_rng(7)
    ia_in, ia_out = [], []
    for k in range(24):
        xi, xf = np.zeros(12), Xf.copy()
        xi[:6] = X0[:6] * (1 + 0.3 * rng.uniform(-1, 1, 6))
        xi[2], xi[3] = rng.uniform(-1.2, 1.2), rng.uniform(-3, 3)
        xf[:6] *= 1 + 0.3 * rng.uniform(-1, 1, 6)
        ti = [0.0, 5.0, T1, 25.0][k % 4]
        ref.set_flags(1, 1 if ti < T1 else 0)
        guess = ref.init_analytical(ti, xi, 40.0, xf)
        if np.all(np.isfinite(guess)):                        # a target behind the horizon has no line of sight: NaN upstream
            ia_in.append(np.concatenate([[ti, 1 if ti < T1 else 0], xi[:6], xf[:6]]))
            ia_out.append(guess)
    assert len(ia_out) >= 12 and {r[0] for r in ia_in} == {0.0, 5.0, T1, 25.0}
    out.update(a_init_in=np.array(ia_in), a_init_out=np.array(ia_out))
    np.savez_compressed(out_path, **out)
    print("rows %d, undecidable %d, chart-change rows %d; wrote %s, %d bytes" % (len(rows), len(und), len(cc), out_path, os.path.getsize(out_path)))
    assert os.path.getsize(out_path) <= 1 << 19


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "interceptor_pin.npz"))
