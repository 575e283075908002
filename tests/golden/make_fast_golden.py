"""Writes tests/golden/fast_pin.npz: the rows, values and bounds that pin the throughput flavour's right-hand sides
(tests/test_fast_pin_cpu.py, tests/test_gpu_fast_pin.py).  Needs mpmath; the tests that read the fixture do not.

    python tests/golden/make_fast_golden.py [out.npz]

Per model (prefix g_ Goddard, c_ covid19): X, t, sw, block (index into *_blocks, the parameter blocks), group (index into
group_names), val (the right-hand side, rounded once to double), Bref / Bfast (bounds of the reference-order / fast-structure
evaluation, tests/fast_reference.py), dec (every branch margin exceeds 4x its error), u / Bu (control) and, for Goddard, H / BH
(Hamiltonian), both in the reference order.  For the undecidable rows (*_und, indices) the same quantities on the other side of the
undecided decisions (*_alt_*).  traj_*: 64 starts, N = 10 RK4 steps in mpf on the mathematical right-hand side, and the
reference-order CPU oracle's own deviation from that (per component, batch maximum).

The kink rows sit a chosen number of error-widths on either side of a decision; at most 2 % of all rows may be undecidable
(asserted below: a condition of the fixture, not a measurement)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

import fast_reference as fr                                   # noqa: E402
from conftest import goddard_costate_batch                    # noqa: E402

G_NOMINAL = [3.5, 7.0, 310.0, 500.0, 1.0, 1.0, 1.0, -1.0]     # C, b, KD, kr, u_max, mu1, mu2, singularControl
C_NOMINAL = [3.4, 14, 5, 1, 0.1, 1, -10, 20]                  # PARAMS of tests/test_gpu_covid.py
C_LARGE_N = [3.4, 14, 5, 6.7e7, 0.1 * 6.7e7, 1, -10, 20]      # unnormalised populations
GROUPS = ["nominal", "iso_rsqrt", "iso_kr0", "iso_rcp", "iso_exp", "air_density", "air_subnormal", "kink",
          "covid", "covid_large_n", "covid_kink"]
KINK_OFFSETS = [-4096, -64, -12, 12, 64, 4096]                # in units of the margin's error: decidable (> 4)
KINK_OFFSETS_CLOSE = [-1, 1]                                  # deliberately inside: the undecidable rows
TRAJ_B, TRAJ_N, TRAJ_TF = 64, 10, 0.078125                    # step 2^-7: the ten steps and their times are exact doubles
REGEN_ROWS = 16


def g_block(**kw):
    names = ["C", "b", "KD", "kr", "u_max", "mu1", "mu2", "singularControl"]
    p = list(G_NOMINAL)
    for k, v in kw.items():
        p[names.index(k)] = v
    return p


def parity_states(B):
    """The states of test_gpu_parity.test_fast_rhs_matches_oracle."""
    rng = np.random.default_rng(11)
    X = goddard_costate_batch(256, 0.3) * (1 + 0.05 * rng.uniform(-1, 1, (256, 14)))
    X[:, 3:6] = rng.uniform(-0.1, 0.1, (256, 3))
    t = rng.uniform(0, 0.12, 256)
    return X[:B], t[:B]


def random_states(B, seed=99):
    """test_gpu_bitwise.random_states."""
    rng = np.random.default_rng(seed)
    X = np.empty((B, 14))
    dirs = rng.normal(size=(B, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    X[:, 0:3] = dirs * rng.uniform(0.98, 1.05, (B, 1))
    X[:, 3:6] = rng.normal(size=(B, 3)) * 10.0 ** rng.uniform(-10, -0.5, (B, 1))
    X[:, 6] = rng.uniform(0.2, 1.0, B)
    X[:, 7:10] = rng.normal(size=(B, 3)) * 5
    X[:, 10:13] = rng.normal(size=(B, 3)) * 10.0 ** rng.uniform(-3, 0.5, (B, 1))
    X[:, 13] = rng.uniform(-0.5, 0.5, B)
    return X, rng.uniform(0.0, 0.12, B)


def goddard_rows():
    rows = []
    SW = [0.0227, 0.08]

    def add(group, P, X, t, sw=None):
        for i in range(len(X)):
            rows.append(dict(group=group, P=list(P), X=np.array(X[i], dtype=float), t=float(np.broadcast_to(t, len(X))[i]),
                             sw=list(SW if sw is None else sw[i])))

    rng = np.random.default_rng(2025)
    # nominal: both state sets under mu2 = 1, 0.2 and 0 (on / singular, closed form and fixed value / off, per-row switching times)
    Xp, tp = parity_states(56)
    Xr, tr = random_states(56)
    for X, t in ((Xp, tp), (Xr, tr)):
        add("nominal", g_block(mu2=1.0), X, t)
        add("nominal", g_block(mu2=0.2), X, t)
        sw = np.stack([rng.uniform(0.005, 0.04, len(X)), rng.uniform(0.05, 0.1, len(X))], axis=1)
        add("nominal", g_block(mu2=0.0), X[:28], t[:28], sw[:28])
        add("nominal", g_block(mu2=0.0, singularControl=0.6), X[28:], t[28:], sw[28:])
    # isolating blocks: one primitive alone in a component
    Xi, ti = random_states(32, seed=7)
    add("iso_rsqrt", g_block(KD=0.0, C=0.0), Xi, ti)                    # dX[3..5] = -x / r^3
    add("iso_kr0", g_block(kr=0.0), Xi, ti)                             # E = 1
    Xt = Xi.copy()
    Xt[:, 13] = rng.uniform(0.3, 0.6, len(Xt))                          # Switch < 0: thrust on, some rows saturated
    Xt[:, 10:13] *= (rng.uniform(0.5, 3.0, len(Xt)) / np.linalg.norm(Xt[:, 10:13], axis=1))[:, None]
    add("iso_rcp", g_block(KD=0.0), Xt, ti)                             # 1/m and 1/|p_v|
    Xe = Xi.copy()
    Xe[:, 0:3] = 0.0
    Xe[np.arange(len(Xe)), np.arange(len(Xe)) % 3] = rng.uniform(0.5, 8.0, len(Xe)) * rng.choice([-1.0, 1.0], len(Xe))
    Xe[:, 3:6] = rng.uniform(-0.3, 0.3, (len(Xe), 3))
    add("iso_exp", g_block(kr=1.0), Xe, ti)                             # exp, argument -(r - 1), r along one axis
    # air density: exp arguments +475 .. -675 at kr = 500, then results that are subnormal (and two that underflow to zero)
    Xa, ta = random_states(96, seed=11)
    radius = np.random.default_rng(12).uniform(0.05, 2.35, len(Xa))
    Xa[:, 0:3] *= (radius / np.linalg.norm(Xa[:, 0:3], axis=1))[:, None]
    add("air_density", G_NOMINAL, Xa, ta)
    Xs, ts = random_states(16, seed=13)
    radius = np.concatenate([np.random.default_rng(14).uniform(2.42, 2.488, 14), [2.5, 2.6]])
    Xs[:, 0:3] *= (radius / np.linalg.norm(Xs[:, 0:3], axis=1))[:, None]
    add("air_subnormal", G_NOMINAL, Xs, ts)
    # kinks of the smooth law: Switch = 0 and Switch = -2 mu2 u_max, a few error-widths on either side
    Xk, tk = random_states(4, seed=17)
    for mu2 in (1.0, 0.2):
        P = g_block(mu2=mu2)
        for target, name in ((0.0, "Switch"), (-2 * mu2 * P[4], "Switch+2mu2umax")):
            for j in range(2):
                X = Xk[2 * (mu2 == 0.2) + j].copy()
                mp = fr.mpf
                npv = fr.mpmath.sqrt(sum(mp(float(q)) ** 2 for q in X[10:13]))
                pm0 = (mp(P[5]) - mp(P[0]) / mp(float(X[6])) * npv - mp(target)) / mp(P[1])      # Switch == target here
                X[13] = float(pm0)
                m = fr.evaluate_row("goddard", P, SW, tk[j], X)["margins"][name]
                err = max(m[1], m[2])
                for k in KINK_OFFSETS + (KINK_OFFSETS_CLOSE if j == 0 else []):
                    Y = X.copy()
                    Y[13] = float(pm0 - mp(k) * mp(err) / mp(P[1]))
                    add("kink", P, [Y], tk[j])
    # the arc boundaries of the bang / singular / off law: t on, one ulp below and one ulp above each switching time
    Xb, _ = parity_states(6)
    sw = [0.0227, 0.08]
    tb = [sw[0], np.nextafter(sw[0], 0.0), np.nextafter(sw[0], 1.0), sw[1], np.nextafter(sw[1], 0.0), np.nextafter(sw[1], 1.0)]
    add("kink", g_block(mu2=0.0), Xb, np.array(tb), [sw] * 6)
    return rows


def covid_rows():
    rows = []
    rng = np.random.default_rng(31)

    def state(P, u_target, i_frac):
        """A state whose unclamped control is u_target and whose I is i_frac * Imax (populations in units of N)."""
        R0, Tinf, Tinc, N, Imax = P[:5]
        I = i_frac * Imax
        E = rng.uniform(0.001, 0.05) * N
        S = rng.uniform(0.5, 0.9) * N - I
        R = N - S - E - I
        pS = rng.normal() * 0.5 / N
        pE = pS + u_target * Tinf * N / (R0 * S * I)
        return np.array([S, E, I, R, pS, pE, rng.normal() * 0.5 / N, rng.normal() * 0.1 / N])

    for group, P in (("covid", C_NOMINAL), ("covid_large_n", C_LARGE_N)):
        for i in range(64):
            # a third clamped low, a third high, a third interior; I on both sides of Imax
            rows.append(dict(group=group, P=list(P), X=state(P, rng.uniform(-30, 40), rng.uniform(0.05, 2.0)), t=0.0, sw=[0.0, 0.0]))
    for P in (C_NOMINAL, C_LARGE_N):
        for target, name in ((P[6], "u-umin"), (P[7], "u-umax")):
            X = state(P, target, 0.7)
            m = fr.evaluate_row("covid", P, [0.0, 0.0], 0.0, X)["margins"][name]
            err = max(m[1], m[2])
            mp = fr.mpf
            S, I, pS = (mp(float(q)) for q in (X[0], X[2], X[4]))
            gain = S * I / mp(P[1]) / mp(P[3]) * mp(P[0])                # du / d(pE)
            pE0 = pS + mp(target) / gain
            for k in KINK_OFFSETS + (KINK_OFFSETS_CLOSE if P is C_NOMINAL else []):
                Y = X.copy()
                Y[5] = float(pE0 + mp(k) * mp(err) / gain)
                rows.append(dict(group="covid_kink", P=list(P), X=Y, t=0.0, sw=[0.0, 0.0]))
        for k in (-3, -1, 0, 1, 3):                                      # I next to Imax, by ulps: I - Imax is exact (Sterbenz)
            X = state(P, rng.uniform(-5, 15), 1.0)
            for _ in range(abs(k)):
                X[2] = np.nextafter(X[2], np.inf if k > 0 else -np.inf)
            rows.append(dict(group="covid_kink", P=list(P), X=X, t=0.0, sw=[0.0, 0.0]))
    return rows


def pack(model, rows, prefix):
    blocks = []
    for r in rows:
        if r["P"] not in blocks:
            blocks.append(r["P"])
    out = {prefix + "blocks": np.array(blocks, dtype=float),
           prefix + "block": np.array([blocks.index(r["P"]) for r in rows], dtype=np.int32),
           prefix + "group": np.array([GROUPS.index(r["group"]) for r in rows], dtype=np.int32),
           prefix + "X": np.array([r["X"] for r in rows]), prefix + "t": np.array([r["t"] for r in rows]),
           prefix + "sw": np.array([r["sw"] for r in rows])}
    ev = [fr.evaluate_row(model, r["P"], r["sw"], r["t"], r["X"]) for r in rows]
    keys = [("val", "value"), ("Bref", "B_ref"), ("Bfast", "B_fast"), ("u", "u"), ("Bu", "B_u")] + \
           ([("H", "H"), ("BH", "B_H")] if model == "goddard" else [])
    for k, src in keys:
        out[prefix + k] = np.array([e[src] for e in ev])
    out[prefix + "dec"] = np.array([e["decidable"] for e in ev])
    und = [i for i, e in enumerate(ev) if not e["decidable"]]
    alt = [fr.evaluate_row(model, rows[i]["P"], rows[i]["sw"], rows[i]["t"], rows[i]["X"], flip=ev[i]["undecided"]) for i in und]
    out[prefix + "und"] = np.array(und, dtype=np.int32)
    for k, src in keys:
        out[prefix + "alt_" + k] = np.array([e[src] for e in alt]).reshape((len(und),) + out[prefix + k].shape[1:])
    return out, ev


def trajectories():
    from oracle.oracle import Oracle, MODEL_GODDARD
    X0 = goddard_costate_batch(TRAJ_B, 0.05)
    sw = [0.0227, 0.08]
    step = TRAJ_TF / TRAJ_N
    assert step * TRAJ_N == TRAJ_TF and step == 2.0 ** -7
    ref = [fr.rk4_mpf("goddard", G_NOMINAL, sw, 0.0, x, step, TRAJ_N) for x in X0]
    o = Oracle(MODEL_GODDARD, step_nbr=TRAJ_N, params=G_NOMINAL)
    Xo = o.integrate_batch(0.0, TRAJ_TF, X0)
    dev = np.array([[fr._up(abs(fr.mpf(float(Xo[b, c])) - ref[b][c])) for c in range(14)] for b in range(TRAJ_B)])
    return {"traj_P": np.array(G_NOMINAL, dtype=float), "traj_X0": X0, "traj_tf": np.array(TRAJ_TF), "traj_N": np.array(TRAJ_N),
            "traj_mpf": np.array([[float(q) for q in row] for row in ref]), "traj_oracle_dev": dev.max(axis=0)}


def regenerate(fix, idx, model):
    """Rows idx of the stored fixture evaluated afresh: [(stored, fresh)] arrays to compare bit for bit."""
    p = "g_" if model == "goddard" else "c_"
    pairs = []
    for i in idx:
        e = fr.evaluate_row(model, fix[p + "blocks"][fix[p + "block"][i]], fix[p + "sw"][i], fix[p + "t"][i], fix[p + "X"][i])
        for k, src in (("val", "value"), ("Bref", "B_ref"), ("Bfast", "B_fast")):
            pairs.append((fix[p + k][i], e[src]))
        pairs.append((np.array(fix[p + "dec"][i]), np.array(e["decidable"])))
    return pairs


def main(out_path):
    out = {"group_names": np.array(GROUPS)}
    g, eg = pack("goddard", goddard_rows(), "g_")
    c, ec = pack("covid", covid_rows(), "c_")
    out.update(g)
    out.update(c)
    out.update(trajectories())
    total = len(eg) + len(ec)
    und = len(g["g_und"]) + len(c["c_und"])
    print("rows: goddard %d, covid %d; undecidable %d (%.2f %%)" % (len(eg), len(ec), und, 100.0 * und / total))
    assert und <= 0.02 * total, "more than 2 % of the rows are undecidable: move the kink offsets"
    assert und > 0, "no undecidable row left: the two-branch test would check nothing"
    np.savez_compressed(out_path, **out)
    print("wrote %s, %d bytes" % (out_path, os.path.getsize(out_path)))
    assert os.path.getsize(out_path) < 1 << 20


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "fast_pin.npz"))
