"""Writes tests/golden/adaptive_models_pin.npz: short adaptive Dormand-Prince segments of the interceptor (with its chart-change hook,
its two phases and the hand-back) and of vtolUAV (with its obstacle map), with the 240-bit replay's accepted times, states and one
derived bound for each (tests/adaptive_models_reference.py; read by tests/test_adaptive_models_pin_cpu.py and
tests/test_gpu_adaptive_models_pin.py).  Needs mpmath; the GPU tests read the fixture only.

    python tests/golden/make_adaptive_models_golden.py [out.npz]

The candidates are walked in a fixed order.  The float64 emulation says which rows of the coverage table a candidate goes through; one
that still fills a row is replayed on Tracked numbers and KEPT ONLY IF EVERY DECISION IS DECIDABLE IN BOTH FLAVOURS (every margin above
DECIDE_FACTOR x its bound: the controller's, the loop's, the chart-limit test before every step, the sign tests of new_angles, every
pivot choice of lu6_solve, every box selection at every stage), both flavours take the same decisions, their 240-bit trajectories
agree to 2^-120, and the replay goes through the same rows.  The file holds decidable scenarios only.  A row of the table left empty
is a failed run (asserted) -- except 1 -> 2 -> 1, which the issue makes conditional: the run says which way it went.

Per model (prefix i_ interceptor, v_ vtolUAV): P, tol, t0, tf, step_nbr, X0 (v_map: index into map_names, with table_<name>); nrows,
phase_rows [2]; times / Bt_ref / Bt_fast [rows]; states / B_ref / B_fast [rows][12] (the last row the end state -- for the interceptor
the handed-back row, whose time is tf itself); stage, chart [rows]; ntrials, err / h / accepted [trials]; branch
[len(branch_names)], flag [len(i_flag_names) / len(v_flag_names)]; pow_ref / pow_fast (the largest share of C_POW in an end-state
bound); trail (text).  Padded with NaN past nrows / ntrials.  The zip members carry a fixed date: a clean run reproduces the file byte
for byte."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import adaptive_models_reference as am                        # noqa: E402
import dopri5_reference as d5                                 # noqa: E402
import interceptor_reference as ir                            # noqa: E402
from make_dopri5_golden import save                           # noqa: E402

PREFIX = {"interceptor": "i_", "vtol": "v_"}
FLAGS = {"interceptor": am.I_FLAGS, "vtol": am.V_FLAGS}
CONTROLLER = ["single_cap", "grow", "keep", "reject", "clamp", "reject2", "reinit"]
OPTIONAL = ["there_and_back"]                                 # kept if a decidable one exists within the trial cap
LIMIT = {"interceptor": 12, "vtol": 10}
MAX_TRIALS = 9
MAPS = ["shipped", "synthetic", "grid256"]                  # the tables the coverage table asks for
I_BASE = [10000, 20, 1.46, 0.3, 0.8, 0.01, 1e-3, 0.1, 1, 0.2, 0.1, 0.1]
VTOL = np.load(os.path.join(HERE, "vtol_pin.npz"))
ALL_MAPS = [str(m) for m in VTOL["map_names"]]
VTOL_ROWS = [0, 513, 608, 610, 689, 700, 891]                 # rows of vtol_pin.npz whose trails visit the controller's branches


def i_block(**kw):
    P = ir.SHIPPED.copy()
    for k, v in kw.items():
        P[getattr(ir, k)] = v
    return P


def i_sc(P, gamma, t0, tf, tol, n):
    X = np.array(I_BASE, dtype=float)
    X[2] = gamma
    return dict(model="interceptor", P=np.array(P, dtype=float), tol=float(tol), t0=float(t0), tf=float(tf), step_nbr=int(n), X0=X)


def v_sc(row, tol, tf, n):
    m = str(VTOL["map_names"][VTOL["map"][row]])
    return dict(model="vtol", P=VTOL["blocks"][VTOL["block"][row]].astype(float), table=VTOL["table_" + m].astype(float), map=m,
                tol=float(tol), t0=0.0, tf=float(tf), step_nbr=int(n), X0=VTOL["X"][row].astype(float))


def interceptor_candidates():
    """gamma = 1.46 crosses the chart limit after a few steps, 1.5 starts beyond it, 0.3 never gets there; PROP / Q = 1/16 and 1/8 put
    t1 inside the segment (powers of two: t1 is exact); chartLimit = 0.995 sends the state there and back."""
    out = []
    blocks = [i_block(), i_block(PROP=1, Q=16), i_block(PROP=1, Q=8), i_block(CHART_LIMIT=0.995)]
    for P in blocks:
        for gamma in (1.46, 1.5, 0.3):
            for t0, tf in ((0, 0.125), (0, 0.25), (0.03125, 0.125), (0, 0.0625), (0.0625, 0.25)):
                for tol in (1e-7, 1e-4, 1e-6, 1e-8, 1e-5):
                    for n in (1, 2):
                        out.append(i_sc(P, gamma, t0, tf, tol, n))
    return out


def vtol_candidates():
    out = []
    for tol in (1e-8, 1e-4):
        for row in VTOL_ROWS:
            out.append(v_sc(row, tol, 0.25, 1))
    moving = np.flatnonzero(VTOL["dec"] & (np.linalg.norm(VTOL["X"][:, 3:6], axis=1) > 0))
    for m in MAPS:
        rows = [r for r in moving if str(VTOL["map_names"][VTOL["map"][r]]) == m]
        for row in rows[:: max(1, len(rows) // (6 if m == "grid256" else 40))]:
            for tol, n in ((1e-8, 1), (1e-6, 2), (1e-10, 1)):
                out.append(v_sc(row, tol, 0.25, n))
    return out


def covered(sc, r, value=float):
    return am.branches(sc, r, value) | am.flags(sc, r) | ({"map:" + sc["map"]} if sc["model"] == "vtol" else set())


def emulated(sc):
    """What the float64 emulation of either flavour goes through, or None where the candidate is too long or not finite."""
    out = set()
    for fl in ("ref", "fast"):
        try:
            _, states, _, r = am.emulate(sc, fl)
        except AssertionError:
            return None
        if "truncated" in r or len(r["trials"]) > MAX_TRIALS or not np.all(np.isfinite(states)):
            return None
        out |= covered(sc, r)
    return out


def needs(model):
    need = {b: 1 for b in CONTROLLER + [f for f in FLAGS[model]]}
    if model == "vtol":
        need.update({"map:" + m: 1 for m in MAPS})
    return need


def select(model, cands):
    need = needs(model)
    have = {b: 0 for b in need}
    chosen = []
    for sc in cands:
        if all(have[b] >= need[b] for b in need) or len(chosen) >= LIMIT[model]:
            break
        cov = emulated(sc)
        if not cov or not any(have.get(b, 1) < need.get(b, 0) for b in cov):
            continue
        ev = am.evaluate(sc)
        if not ev["decidable"]:
            continue
        ev["covered"] = ev["branches"] | ev["flags"] | ({"map:" + sc["map"]} if model == "vtol" else set())
        if not any(have.get(b, 1) < need.get(b, 0) for b in ev["covered"]):
            continue
        for b in ev["covered"]:
            if b in have:
                have[b] += 1
        ev.update({"pow_" + fl: v for fl, v in am.pow_share(sc, ev).items()})
        chosen.append((sc, ev))
        print("  kept %-11s %2d trials: %s" % (model, len(ev["err"]), ev["trail"]))
    short = sorted(b for b in need if have[b] < need[b])
    for b in OPTIONAL:
        if b in short:
            short.remove(b)
            print("  %s: no decidable scenario with %s within %d trials among the candidates: the table drops that row" % (model, b, MAX_TRIALS))
    assert not short, "%s: rows of the coverage table left empty: %s" % (model, short)
    return chosen


def pack(model, chosen):
    p = PREFIX[model]
    R = max(len(ev["times"]) for _, ev in chosen)
    T = max(len(ev["err"]) for _, ev in chosen)

    def pad(a, shape):
        out = np.full(shape, np.nan)
        out[tuple(slice(0, k) for k in np.shape(a))] = a
        return out

    col = lambda f: [f(sc, ev) for sc, ev in chosen]
    out = {p + "P": np.array(col(lambda s, e: s["P"])), p + "tol": np.array(col(lambda s, e: s["tol"])),
           p + "t0": np.array(col(lambda s, e: s["t0"])), p + "tf": np.array(col(lambda s, e: s["tf"])),
           p + "step_nbr": np.array(col(lambda s, e: s["step_nbr"]), dtype=np.int32), p + "X0": np.array(col(lambda s, e: s["X0"])),
           p + "nrows": np.array(col(lambda s, e: len(e["times"])), dtype=np.int32),
           p + "phase_rows": np.array(col(lambda s, e: (e["phase_rows"] + [0])[:2]), dtype=np.int32),
           p + "ntrials": np.array(col(lambda s, e: len(e["err"])), dtype=np.int32),
           p + "times": np.array(col(lambda s, e: pad(e["times"], (R,)))), p + "states": np.array(col(lambda s, e: pad(e["states"], (R, 12)))),
           p + "stage": np.array(col(lambda s, e: pad(e["stage"], (R,)))), p + "chart": np.array(col(lambda s, e: pad(e["chart"], (R,)))),
           p + "err": np.array(col(lambda s, e: pad(e["err"], (T,)))), p + "h": np.array(col(lambda s, e: pad(e["h"], (T,)))),
           p + "accepted": np.array(col(lambda s, e: pad(e["accepted"].astype(float), (T,)))),
           p + "branch": np.array(col(lambda s, e: [b in e["branches"] for b in d5.BRANCHES])),
           p + "flag": np.array(col(lambda s, e: [f in e["flags"] for f in FLAGS[model]])),
           p + "trail": np.array(col(lambda s, e: e["trail"]))}
    for fl in ("ref", "fast"):
        out[p + "Bt_" + fl] = np.array(col(lambda s, e: pad(e["Bt_" + fl], (R,))))
        out[p + "B_" + fl] = np.array(col(lambda s, e: pad(e["B_" + fl], (R, 12))))
        out[p + "pow_" + fl] = np.array(col(lambda s, e: e["pow_" + fl]))
    if model == "vtol":
        out[p + "map"] = np.array(col(lambda s, e: ALL_MAPS.index(s["map"])), dtype=np.int32)
    return out


def scenario(fix, model, i):
    """Scenario i of a model as the dict adaptive_models_reference.run / evaluate take."""
    p = PREFIX[model]
    sc = dict(model=model, P=fix[p + "P"][i].astype(float), tol=float(fix[p + "tol"][i]), t0=float(fix[p + "t0"][i]),
              tf=float(fix[p + "tf"][i]), step_nbr=int(fix[p + "step_nbr"][i]), X0=fix[p + "X0"][i].astype(float))
    if model == "vtol":
        sc["map"] = str(fix["map_names"][fix[p + "map"][i]])
        sc["table"] = fix["table_" + sc["map"]].astype(float)
    return sc


def regenerate(fix, model, idx):
    """Scenarios idx of the stored fixture evaluated afresh: [(stored, fresh)] arrays to compare bit for bit."""
    p = PREFIX[model]
    pairs = []
    for i in idx:
        ev = am.evaluate(scenario(fix, model, i))
        pairs.append((np.array(True), np.array(ev["decidable"])))
        r = len(ev["times"])
        pairs.append((np.array(fix[p + "nrows"][i]), np.array(r)))
        for k in ("times", "states", "stage", "chart", "Bt_ref", "Bt_fast", "B_ref", "B_fast"):
            pairs.append((fix[p + k][i][:r], ev[k]))
        pairs.append((fix[p + "err"][i][:len(ev["err"])], ev["err"]))
    return pairs


def ratios(got, val, B):
    err = np.abs(got - val)
    with np.errstate(all="ignore"):
        return np.where(err == 0, 0.0, np.where(np.isnan(err), np.inf, err / B))


def main(out_path):
    out = {"branch_names": np.array(d5.BRANCHES), "i_flag_names": np.array(am.I_FLAGS), "v_flag_names": np.array(am.V_FLAGS),
           "map_names": np.array(ALL_MAPS), "c_pow": np.array(d5.C_POW), "decide_factor": np.array(d5.DECIDE_FACTOR)}
    for m in ALL_MAPS:
        out["table_" + m] = VTOL["table_" + m]
    for model, cands in (("interceptor", interceptor_candidates()), ("vtol", vtol_candidates())):
        print(model)
        chosen = select(model, cands)
        out.update(pack(model, chosen))
        p = PREFIX[model]
        print("  %d scenarios, up to %d rows and %d trial steps" % (len(chosen), out[p + "nrows"].max(), out[p + "ntrials"].max()))
        print("  branches: %s" % " ".join("%s=%d" % (b, c) for b, c in zip(d5.BRANCHES, out[p + "branch"].sum(axis=0))))
        print("  coverage: %s" % " ".join("%s=%d" % (b, c) for b, c in zip(FLAGS[model], out[p + "flag"].sum(axis=0))))
        for fl in ("ref", "fast"):
            top = 0.0
            for i, (sc, ev) in enumerate(chosen):
                t, s, _, _ = am.emulate(sc, fl)
                top = max(top, ratios(t, ev["times"], ev["Bt_" + fl]).max(), ratios(s, ev["states"], ev["B_" + fl]).max())
            B, X = out[p + "B_" + fl], out[p + "states"]
            rel = max(np.nanmax(B[i] / np.nanmax(np.abs(X[i]), axis=0)) for i in range(len(X)))
            print("  %-4s float64 replay, largest err/bound %.3f; largest bound / component scale %.3g; largest share of C_POW in an "
                  "end-state bound %.3g" % (fl, top, rel, out[p + "pow_" + fl].max()))
            assert top <= 1.0
    save(out_path, out)
    print("wrote %s, %d bytes" % (out_path, os.path.getsize(out_path)))
    assert os.path.getsize(out_path) <= 235000


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "adaptive_models_pin.npz"))
