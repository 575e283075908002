"""The interceptor and vtolUAV under the adaptive Dormand-Prince integrator, replayed over the number kits (helper of
test_adaptive_models_pin_cpu.py, test_gpu_adaptive_models_pin.py and golden/make_adaptive_models_golden.py, not a test).  Nothing
here is new arithmetic: the loop is dopri5_reference.replay, the interceptor's right-hand sides and chart change are
interceptor_reference's, vtolUAV's right-hand sides and map are vtol_reference's.  This module is their composition.

  interceptor_adaptive  InterceptorT::compute_traj<1> (socp_amd/csrc/models_interceptor.hpp) and orc_interceptor_compute_traj_adaptive
                        (oracle/interceptor_oracle.c) statement for statement: chart = 1; t1 = PROP / Q in double; one or two phases
                        with stage 1 then 0; each phase one integrate_dopri5 whose hook is set_chart, called before every step; the
                        state handed back by ConversionState21 when the chart is 2 at the end.  Rows as the trace reports them: the
                        phase start, one row after every accepted step, the handed-back row; each with t, the raw-chart X, stage, chart.
  vtol_adaptive         integrate_dopri5 over vtol_ref / vtol_fast with the lifted obstacle table as the auxiliary.

Decisions: those of the replay, and under the prefix H<n>. of the n-th hook call the chart-limit test, the sign tests of new_angles and
every pivot choice of lu6_solve (named pivot<k>@H<n>.); the hand-back's under @back.  They all enter the decidability verdict.

MUTATIONS are deliberately wrong compositions for the instrument's own test (test_adaptive_models_pin_cpu.py)."""
import numpy as np

import dopri5_reference as d5
import fast_reference as fr
import interceptor_reference as ir
import vtol_reference as vr
from fast_reference import F64, C_EXP_LIB, mpf

I_MUTATIONS = {
    "stale_k1": "k1 kept across a chart change",
    "hook_once": "the hook called only at the start of a phase",
    "h0_from_t0": "the second phase's first step from tf - t0",
    "stage_kept": "stage stays 1 after t1",
    "no_handback": "the final chart change dropped",
    "chart_reset": "the chart set back to 1 at the second phase",
}
V_MUTATIONS = {
    "table_row_dropped": "the last obstacle missing in stages 2 to 7 only",
}
# two_phase_split: two phases with step_nbr > 1 -- with step_nbr = 1 a first step of the wrong length overshoots the phase and is
# re-formed as tf - t, so nothing would tell (tf - t0) / step_nbr from (tf - t1) / step_nbr
I_FLAGS = ["start_change", "late_change", "there_and_back", "handback", "two_phase", "two_phase_split", "t0_positive", "reject_after_change"]
V_FLAGS = ["kink", "alphaV"]
MAX_TRIALS = 20                                       # two phases of at most about 9 trials


def interceptor_adaptive(K, P, step_nbr, tol, t0, tf, X0, form="ref", mut=None):
    """Returns the replay's result dict; times / states / aux[(stage, chart)] are the trace's rows, `phase_rows` the number of rows
    of each phase and `final` the handed-back state (the last row)."""
    assert mut is None or mut in I_MUTATIONS, mut
    Pk = [K.lift(p) for p in P]
    chart = 1
    t0, tf = float(t0), float(tf)
    t1 = float(F64(P[ir.PROP]) / F64(P[ir.Q]))
    two = t0 < t1 and tf > t1
    stage = 1 if t0 < t1 else 0
    fn = ir.rhs_fast if form == "fast" else (lambda *a: ir.rhs_ref(*a)[0])

    def rhs(K_, t, X, aux):
        return fn(K_, Pk, aux[1], aux[0], t, X)

    def make_hook():
        calls = [0]

        def hook(K_, t, X, aux):
            calls[0] += 1
            if mut == "hook_once" and calls[0] > 1:
                return False, X, aux
            new_chart, Xn = ir.set_chart(K_, Pk, aux[1], X, "@" + K_.prefix)
            return new_chart != aux[1], Xn, (aux[0], new_chart)
        return hook

    r, X, phase_rows = None, X0, []
    for ph in range(2 if two else 1):
        ta = t0 if ph == 0 else t1
        tb = t1 if (two and ph == 0) else tf
        if ph == 1:
            if mut != "stage_kept":
                stage = 0
            if mut == "chart_reset":
                chart = 1
        before = 0 if r is None else len(r["times"])
        r = d5.replay(K, None, None, None, None, tol, tb, step_nbr, X, mut="stale_k1" if mut == "stale_k1" else None, t0=ta, rhs=rhs,
                      aux=(stage, chart), hook=make_hook(), resume=r, h0_from=t0 if (mut == "h0_from_t0" and ph == 1) else None,
                      max_trials=MAX_TRIALS)
        phase_rows.append(len(r["times"]) - before)
        X = r["states"][-1]
        stage, chart = r["aux"][-1]
        if "truncated" in r:
            break
    if chart == 2 and mut != "no_handback":
        X = ir.change_chart(K, Pk, False, X, None, "@back")
    r["times"].append(K.lift(tf))                     # the trace's extra row carries the segment's end time itself
    r["states"].append(X)
    r["aux"].append((stage, chart))
    r["phase_rows"] = phase_rows
    r["final"] = X
    return r


def vtol_adaptive(K, P, table, step_nbr, tol, tf, X0, form="ref", mut=None):
    assert mut is None or mut in V_MUTATIONS, mut
    Pk, tab = [K.lift(p) for p in P], vr.lift_table(K, table)
    fn = vr.vtol_fast if form == "fast" else vr.vtol_ref

    def rhs(K_, t, X, aux):
        if mut == "table_row_dropped" and K_.prefix.split(".")[-2] != "k1":
            aux = aux[:-1]
        d = fn(K_, Pk, aux, X, want_h=False)[0]
        assert not any(q is None for q in d), "a row where the reference is itself NaN (vtolUAV at rest)"
        return d

    with fr.second_order_products():
        return d5.replay(K, None, None, None, None, tol, tf, step_nbr, X0, rhs=rhs, aux=tab, max_trials=MAX_TRIALS)


def run(K, sc, form, mut=None):
    """A scenario (dict: model, P, tol, t0, tf, step_nbr, X0 and, for vtolUAV, table) on a kit."""
    if sc["model"] == "interceptor":
        return interceptor_adaptive(K, sc["P"], sc["step_nbr"], sc["tol"], sc["t0"], sc["tf"], sc["X0"], form, mut)
    assert sc["t0"] == 0.0
    return vtol_adaptive(K, sc["P"], sc["table"], sc["step_nbr"], sc["tol"], sc["tf"], sc["X0"], form, mut)


def emulate(sc, form, mut=None):
    """The composition in numpy.float64: (times[rows], states[rows][12], aux[rows][2] (interceptor: stage, chart), result dict)."""
    with np.errstate(all="ignore"):
        r = run(d5.D5F64(), sc, form, mut)
    aux = np.array([a for a in r["aux"]], dtype=F64) if sc["model"] == "interceptor" else np.zeros((len(r["times"]), 2))
    return np.array(r["times"], dtype=F64), np.array(r["states"], dtype=F64), aux, r


def _vtol_kink(name):
    return name.startswith("h>=0")


def flags(sc, r):
    """The rows of the coverage table beside the controller's branches (names of I_FLAGS / V_FLAGS)."""
    out = set()
    if sc["model"] == "vtol":
        if sc["P"][vr.I_ALPHAV] != 0:
            out.add("alphaV")
        return out
    acc = [x["accepted"] for x in r["trials"]]
    changes = [T for changed, T in r["hooks"] if changed]
    if r["hooks"] and r["hooks"][0][0]:
        out.add("start_change")
    if any(any(acc[:T]) for T in changes):
        out.add("late_change")
    if len(changes) >= 2:
        out.add("there_and_back")
    if r["aux"][-1][1] == 2:
        out.add("handback")
    if len(r["phase_rows"]) == 2 and all(n >= 2 for n in r["phase_rows"]):
        out.add("two_phase")
        if sc["step_nbr"] > 1:
            out.add("two_phase_split")
    if sc["t0"] > 0 and len(r["phase_rows"]) == 1:
        out.add("t0_positive")
    if any(T < len(acc) and not acc[T] for T in changes):
        out.add("reject_after_change")
    return out


def branches(sc, r, value=float):
    return d5.branches(r, sc["step_nbr"], value=value, kinks=_vtol_kink if sc["model"] == "vtol" else ())


def trail(sc, r, value=float):
    """The decision trail as text: one entry per trial step, a chart change (X) where the hook made one, | between the phases."""
    changes = {T for changed, T in r["hooks"] if changed}
    out = []
    for T, x in enumerate(r["trials"]):
        if T in changes:
            out.append("X")
        out.append("%s(h=%.3g err=%.3g)" % ("A" if x["accepted"] else "R", value(x["h"]), value(x["err"])))
    if sc["model"] == "interceptor":
        out.append("rows %s end chart %d" % ("+".join(str(n) for n in r["phase_rows"]), r["aux"][-1][1]))
    return " ".join(out)


def evaluate(sc, c_pow=d5.C_POW):
    """One scenario through the Tracked replay of both flavours.  Returns a dict: times, Bt_ref / Bt_fast [rows]; states, B_ref /
    B_fast [rows][12] (the last row the end state; for the interceptor the handed-back row); stage, chart [rows]; phase_rows; err, h,
    accepted [trials]; decidable, undecided (names, of both flavours); branches, flags; trail."""
    runs = {}
    for fl in ("ref", "fast"):
        K = d5.D5Tracked(c_pow=c_pow, c_exp=C_EXP_LIB if (sc["model"] == "vtol" and fl == "fast") else fr.C_EXP)
        runs[fl] = (K, run(K, sc, fl))
    K, r = runs["ref"]
    Kf, rf = runs["fast"]
    assert not any("truncated" in rr for _, rr in runs.values()), "scenario too long"
    out = {"undecided": sorted(set(K.undecided()) | set(Kf.undecided()))}
    out["decidable"] = not out["undecided"]
    # the two flavours take the same decisions ...
    same = ([x["accepted"] for x in rf["trials"]] == [x["accepted"] for x in r["trials"]] and rf["hooks"] == r["hooks"]
            and len(rf["times"]) == len(r["times"]))
    if sc["model"] == "interceptor":
        same = same and rf["aux"] == r["aux"]
    out["same_decisions"] = same
    if not same:
        out["decidable"] = False
        return out
    # ... and, being the same function, their 240-bit trajectories agree far below a double's spacing
    assert all(abs(p.v - s.v) <= mpf(2) ** -120 * (abs(p.v) + abs(s.v)) + mpf(2) ** -1000
               for rp, rs in zip(r["states"] + [r["times"]], rf["states"] + [rf["times"]]) for p, s in zip(rp, rs)), "the two restatements disagree"
    out["times"], out["Bt_ref"] = d5._pin(K, r["times"])
    out["Bt_fast"] = d5._pin(Kf, rf["times"])[1]
    vals, bnds = zip(*[d5._pin(K, row) for row in r["states"]])
    valf, bndf = zip(*[d5._pin(Kf, row) for row in rf["states"]])
    out["states"], out["B_ref"], out["B_fast"] = np.array(vals), np.array(bnds), np.array(bndf)
    assert np.array_equal(out["states"], np.array(valf)), "the two restatements round to different doubles"
    if sc["model"] == "interceptor":
        out["stage"] = np.array([a[0] for a in r["aux"]], dtype=F64)
        out["chart"] = np.array([a[1] for a in r["aux"]], dtype=F64)
        out["phase_rows"] = list(r["phase_rows"])
    else:
        out["stage"] = out["chart"] = np.zeros(len(r["times"]))
        out["phase_rows"] = [len(r["times"])]
    tr = r["trials"]
    out["err"] = np.array([float(x["err"].v) for x in tr])
    out["h"] = np.array([float(x["h"].v) for x in tr])
    out["accepted"] = np.array([x["accepted"] for x in tr])
    value = lambda e: float(e.v)
    out["branches"] = branches(sc, r, value) | (branches(sc, rf, value) & {"kink"})       # `pos` exists in the throughput flavour only
    out["flags"] = flags(sc, r) | ({"kink"} & out["branches"])
    out["trail"] = trail(sc, r, value)
    return out


def pow_share(sc, ev):
    """The largest share of an end-state bound that comes from C_POW, per flavour."""
    e0 = evaluate(sc, c_pow=0)
    out = {}
    for fl in ("ref", "fast"):
        b, b0 = ev["B_" + fl][-1], e0["B_" + fl][-1]
        with np.errstate(all="ignore"):
            out[fl] = float(np.max(np.where(b > 0, (b - b0) / b, 0.0)))
    return out
