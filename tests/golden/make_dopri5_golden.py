"""Writes tests/golden/dopri5_pin.npz: short adaptive Dormand-Prince segments with the 240-bit replay's accepted times, states, end
state and one derived bound for each (tests/dopri5_reference.py; read by tests/test_dopri5_pin_cpu.py and
tests/test_gpu_dopri5_pin.py).  Needs mpmath; the GPU tests read the fixture only.

    python tests/golden/make_dopri5_golden.py [out.npz]

A scenario is (model, parameter block, switching times, tol, t0 = 0, tf, step_nbr, X0).  The candidates below are walked in a fixed
order; the float64 emulation says which rows of the controller's branch table a candidate goes through, and a candidate that still
fills a row is replayed on Tracked numbers and KEPT ONLY IF EVERY DECISION IS DECIDABLE, in every flavour of its model, and the
replay goes through the same rows.  The file holds decidable scenarios only.  Fewer than QUOTA scenarios in a row of the table
is a failed run (asserted), not a skip.

Per model (prefix g_ Goddard, c_ covid19, d_ double integrator, a_ its 156-element augmented state): P, sw, tol, tf, step_nbr, X0;
nrows, times / Bt_ref / Bt_fast [rows], states / B_ref / B_fast [rows][n] (row 0 the start, the last row the end state; padded with
NaN past nrows); ntrials, err / h / accepted [trials]; n_accepted, n_rejected; branch [len(BRANCHES)] (which rows of the table);
pow_ref / pow_fast: the largest share of an end-state bound that comes from C_POW; trail (text); group (0 = table, 1 = the
augmented start scaled by 1e6, 2 = by 1e-6).  The zip members carry a fixed date, so that a clean run reproduces the file byte
for byte."""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

import dopri5_reference as d5                                 # noqa: E402
from conftest import goddard_costate_batch, GODDARD_TF        # noqa: E402

PREFIX = {"goddard": "g_", "covid": "c_", "dint": "d_", "dint_aug": "a_"}
QUOTA = {"goddard": 4, "covid": 1, "dint": 2, "dint_aug": 2}
TABLE = ["single_cap", "grow", "keep", "reject", "clamp", "reject2", "reinit", "kink"]      # QUOTA each; reinit_reject, grow_04: one case
MAX_TRIALS = 9                                                # "at most about 8 trial steps"
TOLS = [1e-3, 5e-4, 2e-4, 1e-4, 5e-5, 2e-5, 1e-5, 5e-6, 2e-6, 1e-6]
G_NOMINAL = [3.5, 7.0, 310.0, 500.0, 1.0, 1.0, 1.0, -1.0]     # C, b, KD, kr, u_max, mu1, mu2, singularControl
C_NOMINAL = [3.4, 14, 5, 1, 0.1, 1, -10, 20]                  # R0, Tinf, Tinc, N, Imax, muI, umin, umax
C_QUICK = [3.4, 0.14, 0.05, 1, 0.1, 1, -10, 20]                 # the same epidemic on a clock 100 times faster: steps get rejected
D_NOMINAL = [1.0, 1.0, 0.01]                                  # u_max, a_max, muT


def g_block(**kw):
    p = list(G_NOMINAL)
    for k, v in kw.items():
        p[["C", "b", "KD", "kr", "u_max", "mu1", "mu2", "singularControl"].index(k)] = v
    return p


def sc(model, P, sw, tol, tf, n, X0):
    return dict(model=model, P=[float(p) for p in P], sw=[float(s) for s in sw], tol=float(tol), tf=float(tf), step_nbr=int(n),
                X0=np.array(X0, dtype=float))


def goddard_candidates():
    X0 = goddard_costate_batch(4, 1e-3)
    # states further along the nominal flight (rounded to 7 digits: they are inputs, not results)
    later = []
    for t_at in (0.05, 0.12, 0.2):
        st = d5.emulate("goddard", "ref", G_NOMINAL, [0.0227, 0.08], 1e-8, t_at, 4, X0[0])[1][-1]
        later.append(np.array([float("%.7g" % v) for v in st]))
    out = []
    # first the bang / singular / off law (mu2 = 0): a switching time inside the segment (fixed singular values keep the jump small or large)
    for sing in (0.99, 0.9, -1.0):
        for sw0 in (0.0031, 0.0047, 0.0101):
            for tf in (sw0 * 1.25, sw0 * 1.6, sw0 * 2.5):
                for n in (1, 2, 3):
                    for tol in (1e-3, 2e-4, 5e-5):
                        out.append(sc("goddard", g_block(mu2=0.0, singularControl=sing), [sw0, 0.2], tol, tf, n, X0[2]))
    # then the smooth law (mu2 > 0)
    for tf in (GODDARD_TF / 64, GODDARD_TF / 32, GODDARD_TF / 16, GODDARD_TF / 8, GODDARD_TF / 4, GODDARD_TF / 2, 0.2):
        for n in (1, 2, 3, 4):
            for tol in TOLS:
                for P in (G_NOMINAL, g_block(mu2=0.2)):
                    for X in list(X0[:2]) + later:
                        out.append(sc("goddard", P, [0.0227, 0.08], tol, tf, n, X))
    return out


def covid_candidates():
    N = 1.0
    base = np.array([0.70, 0.05, 0.06, 0.19, 0.4, 0.9, -0.3, 0.1])
    near = np.array([0.70, 0.08, 0.0995, 0.1205, 0.4, 0.9, -0.3, 0.1])          # I below Imax and rising through it
    clamp = np.array([0.70, 0.05, 0.06, 0.19, 0.4, 0.4 + 19.9 * 14 / (3.4 * 0.70 * 0.06), -0.3, 0.1])      # u just under umax
    out = []
    for P in (C_NOMINAL, C_QUICK):
        for X in (base, near, clamp):
            for tf in (0.03125, 0.05, 0.0625, 0.08, 0.1, 0.125, 0.15, 0.2, 0.25):
                for n in (1, 2, 3, 4):
                    for tol in TOLS:
                        out.append(sc("covid", P, [0.0, 0.0], tol, tf, n, X * N))
    return out


def dint_states():
    out = []
    for s in (2.0, 5.0, 10.0, 20.0, 30.0, 40.0, 50.0, 70.0, 100.0, 200.0):                               # |p_r| / |p_v|: how fast the saturated thrust turns
        X = np.zeros(12)
        X[0:3] = [0.3, -0.2, 0.1]
        X[3:6] = [0.1, 0.05, -0.08]
        X[6:9] = np.array([0.5, -0.3, 0.2]) * s
        X[9:12] = [1.5, -1.0, 0.8]
        out.append(X)
    for s in (1.0, 4.0):                                                    # |p_v| falls through u_max a_max: the saturation kink
        X = np.zeros(12)
        X[3:6] = [0.1, 0.05, -0.08]
        X[6:9] = np.array([1.0, 0.1, -0.2]) * s
        X[9:12] = [1.04, 0.05, 0.1]
        out.append(X)
    return out


def dint_candidates(model):
    out = []
    for X in dint_states():
        if model == "dint_aug":
            X = np.concatenate([X, np.eye(12).ravel()])
        for tf in (0.03125, 0.05, 0.0625, 0.08, 0.1, 0.125, 0.15, 0.2, 0.25):
            for n in (1, 2, 3, 4):
                for tol in TOLS:
                    out.append(sc(model, D_NOMINAL, [0.0, 0.0], tol, tf, n, X))
    return out


def emulated_branches(s):
    with np.errstate(all="ignore"):
        r = d5.replay(d5.D5F64(), s["model"], "ref", s["P"], s["sw"], s["tol"], s["tf"], s["step_nbr"], s["X0"])
    if "truncated" in r or len(r["trials"]) > MAX_TRIALS:
        return None
    if s["model"] in ("dint", "dint_aug"):
        # the unsaturated double integrator is a polynomial of degree <= 3: Dormand-Prince integrates it exactly and err is
        # rounding noise.  Only scenarios that start saturated are used.
        if not r["trials"][0]["start_taken"].get("norm_u-u_max", False):
            return None
    return d5.branches(r, s["step_nbr"])


def evaluate(s):
    ev = d5.evaluate_scenario(s)
    if ev["decidable"]:
        e0 = d5.evaluate_scenario(s, c_pow=0)
        for fl in d5.FLAVOURS[s["model"]]:
            b, b0 = ev["B_" + fl][-1], e0["B_" + fl][-1]
            with np.errstate(all="ignore"):
                ev["pow_" + fl] = float(np.max(np.where(b > 0, (b - b0) / b, 0.0)))
    return ev


def select(model, cands):
    need = {b: QUOTA[model] for b in TABLE}
    need["reinit_reject"] = 1
    need["grow_04"] = 1                                       # what tells a growth threshold of 0.4 from 0.5
    have = {b: 0 for b in need}
    chosen = []
    for s in cands:
        if all(have[b] >= need[b] for b in need):
            break
        br = emulated_branches(s)
        if not br or not any(b in need and have[b] < need[b] for b in br):
            continue
        ev = evaluate(s)
        if not ev["decidable"] or not any(b in need and have[b] < need[b] for b in ev["branches"]):
            continue
        for b in ev["branches"]:
            if b in have:
                have[b] += 1
        chosen.append((s, ev, 0))
    short = {b: (have[b], need[b]) for b in need if have[b] < need[b]}
    assert not short, "%s: rows of the branch table below their minimum (have, need): %s" % (model, short)
    return chosen


def scaled_variants(chosen):
    """One augmented scenario with the sensitivity part of X0 scaled by 1e6 and by 1e-6: the denominators of the error norm move
    across lanes and k slots of the wave kernel."""
    out = []
    for s, ev, _ in chosen:
        if len(ev["accepted"]) >= 3 and not ev["accepted"].all():
            for g, f in ((1, 1e6), (2, 1e-6)):
                t = dict(s, X0=np.concatenate([s["X0"][:12], s["X0"][12:] * f]))
                e = evaluate(t)
                assert e["decidable"], (f, e["undecided"])
                out.append((t, e, g))
            return out
    raise AssertionError("no augmented scenario with a rejection to scale")


def pack(model, chosen):
    p = PREFIX[model]
    n = len(chosen[0][0]["X0"])
    R = max(len(ev["times"]) for _, ev, _ in chosen)
    T = max(len(ev["err"]) for _, ev, _ in chosen)
    fls = d5.FLAVOURS[model]

    def pad(a, shape):
        out = np.full(shape, np.nan)
        out[tuple(slice(0, k) for k in np.shape(a))] = a
        return out

    out = {p + "P": np.array([s["P"] for s, _, _ in chosen]), p + "sw": np.array([s["sw"] for s, _, _ in chosen]),
           p + "tol": np.array([s["tol"] for s, _, _ in chosen]), p + "tf": np.array([s["tf"] for s, _, _ in chosen]),
           p + "step_nbr": np.array([s["step_nbr"] for s, _, _ in chosen], dtype=np.int32),
           p + "X0": np.array([s["X0"] for s, _, _ in chosen]),
           p + "group": np.array([g for _, _, g in chosen], dtype=np.int32),
           p + "nrows": np.array([len(ev["times"]) for _, ev, _ in chosen], dtype=np.int32),
           p + "ntrials": np.array([len(ev["err"]) for _, ev, _ in chosen], dtype=np.int32),
           p + "n_accepted": np.array([ev["n_accepted"] for _, ev, _ in chosen], dtype=np.int32),
           p + "n_rejected": np.array([ev["n_rejected"] for _, ev, _ in chosen], dtype=np.int32),
           p + "times": np.array([pad(ev["times"], (R,)) for _, ev, _ in chosen]),
           p + "states": np.array([pad(ev["states"], (R, n)) for _, ev, _ in chosen]),
           p + "err": np.array([pad(ev["err"], (T,)) for _, ev, _ in chosen]),
           p + "h": np.array([pad(ev["h"], (T,)) for _, ev, _ in chosen]),
           p + "accepted": np.array([pad(ev["accepted"].astype(float), (T,)) for _, ev, _ in chosen]),
           p + "branch": np.array([[b in ev["branches"] for b in d5.BRANCHES] for _, ev, _ in chosen]),
           p + "trail": np.array([ev["trail"] for _, ev, _ in chosen])}
    for fl in fls:
        out[p + "Bt_" + fl] = np.array([pad(ev["Bt_" + fl], (R,)) for _, ev, _ in chosen])
        out[p + "B_" + fl] = np.array([pad(ev["B_" + fl], (R, n)) for _, ev, _ in chosen])
        out[p + "pow_" + fl] = np.array([ev["pow_" + fl] for _, ev, _ in chosen])
    return out


def scenario(fix, model, i):
    """Scenario i of a model as the dict evaluate_scenario / emulate take."""
    p = PREFIX[model]
    return sc(model, fix[p + "P"][i], fix[p + "sw"][i], fix[p + "tol"][i], fix[p + "tf"][i], fix[p + "step_nbr"][i], fix[p + "X0"][i])


def regenerate(fix, model, idx):
    """Scenarios idx of the stored fixture evaluated afresh: [(stored, fresh)] arrays to compare bit for bit."""
    p = PREFIX[model]
    pairs = []
    for i in idx:
        ev = d5.evaluate_scenario(scenario(fix, model, i))
        r = len(ev["times"])
        pairs.append((np.array(fix[p + "nrows"][i]), np.array(r)))
        pairs.append((fix[p + "times"][i][:r], ev["times"]))
        pairs.append((fix[p + "states"][i][:r], ev["states"]))
        for fl in d5.FLAVOURS[model]:
            pairs.append((fix[p + "B_" + fl][i][:r], ev["B_" + fl]))
            pairs.append((fix[p + "Bt_" + fl][i][:r], ev["Bt_" + fl]))
        pairs.append((fix[p + "err"][i][:len(ev["err"])], ev["err"]))
        pairs.append((np.array(True), np.array(ev["decidable"])))
    return pairs


def save(path, arrays):
    """An .npz whose bytes depend on the arrays alone (numpy.savez stamps the members with the time of day)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main(out_path):
    out = {"branch_names": np.array(d5.BRANCHES), "c_pow": np.array(d5.C_POW), "decide_factor": np.array(d5.DECIDE_FACTOR)}
    cands = {"goddard": goddard_candidates(), "covid": covid_candidates(), "dint": dint_candidates("dint"),
             "dint_aug": dint_candidates("dint_aug")}
    for model in ("goddard", "covid", "dint", "dint_aug"):
        chosen = select(model, cands[model])
        if model == "dint_aug":
            chosen += scaled_variants(chosen)
        out.update(pack(model, chosen))
        p = PREFIX[model]
        print("%-9s %d scenarios, up to %d rows and %d trial steps" % (model, len(chosen), out[p + "nrows"].max(), out[p + "ntrials"].max()))
        for fl in d5.FLAVOURS[model]:
            counts = out[p + "branch"][out[p + "group"] == 0].sum(axis=0)
            B, X = out[p + "B_" + fl], out[p + "states"]
            rel = []
            for i in range(len(X)):
                r = out[p + "nrows"][i]
                rel.append(np.max(B[i, :r] / np.max(np.abs(X[i, :r]))))
            print("  %-4s per branch: %s" % (fl, " ".join("%s=%d" % (b, c) for b, c in zip(d5.BRANCHES, counts))))
            print("  %-4s largest bound / state scale %.3g; largest time bound / tf %.3g; largest share of C_POW in an end-state bound %.3g"
                  % (fl, max(rel), np.nanmax(out[p + "Bt_" + fl] / out[p + "tf"][:, None]), out[p + "pow_" + fl].max()))
    save(out_path, out)
    print("wrote %s, %d bytes" % (out_path, os.path.getsize(out_path)))
    assert os.path.getsize(out_path) < 1 << 20


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "dopri5_pin.npz"))
