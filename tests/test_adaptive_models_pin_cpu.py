"""CPU: the instrument that pins the interceptor and vtolUAV under the adaptive Dormand-Prince integrator
(tests/adaptive_models_reference.py, tests/golden/adaptive_models_pin.npz) is itself checked before any kernel is judged by it.

  * the fixture fills its coverage table with decidable scenarios (the generator asserts the same table);
  * the composition in numpy.float64 (D5F64 over the F64 kits) meets every bound of every row, factor 1, and reproduces the
    fixture's row counts, stage and chart columns exactly;
  * the CPU oracle (orc_interceptor_compute_traj_adaptive) meets the reference-order bound on the end state of every interceptor
    scenario;
  * every deliberately wrong composition (adaptive_models_reference.I_MUTATIONS, V_MUTATIONS) VIOLATES a bound of at least one scenario
    BY A FACTOR >= 10 -- the bar test_dopri5_pin_cpu.test_mutated_replays_violate_a_bound_tenfold sets.  Beside it the test prints what
    the earlier comparison (against the CPU restatement at 100 x tol, relative to max(1, |x|)) makes of the same mutated replay;
  * with mpmath present, two scenarios per model evaluated afresh equal the stored fixture bit for bit."""
import os
import sys

import numpy as np
import pytest

import adaptive_models_reference as am
import dopri5_reference as d5
from oracle.oracle import Oracle, MODEL_INTERCEPTOR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "adaptive_models_pin.npz"))
PREFIX = {"interceptor": "i_", "vtol": "v_"}
MODELS = list(PREFIX)
BRANCHES = [str(b) for b in FIX["branch_names"]]
FLAGS = {"interceptor": [str(f) for f in FIX["i_flag_names"]], "vtol": [str(f) for f in FIX["v_flag_names"]]}
CONTROLLER = ["single_cap", "grow", "keep", "reject", "clamp", "reject2", "reinit"]
MUTATIONS = [("interceptor", m) for m in am.I_MUTATIONS] + [("vtol", m) for m in am.V_MUTATIONS]

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
try:
    import make_adaptive_models_golden as gen
finally:
    sys.path.pop(0)


def ratios(got, val, B):
    """|got - val| / B per component, 0 where they are equal (a bound of zero demands equality)."""
    err = np.abs(got - val)
    with np.errstate(all="ignore"):
        return np.where(err == 0, 0.0, np.where(np.isnan(err), np.inf, err / B))


def worst(model, i, fl, times, states):
    """The largest |got - value| / bound over the rows a replay shares with the fixture (times and states)."""
    p = PREFIX[model]
    r = min(len(times), int(FIX[p + "nrows"][i]))
    return max(ratios(times[:r], FIX[p + "times"][i][:r], FIX[p + "Bt_" + fl][i][:r]).max(),
               ratios(states[:r], FIX[p + "states"][i][:r], FIX[p + "B_" + fl][i][:r]).max())


def test_fixture_fills_the_coverage_table_with_decidable_scenarios():
    assert int(FIX["c_pow"]) == d5.C_POW and int(FIX["decide_factor"]) == d5.DECIDE_FACTOR and BRANCHES == d5.BRANCHES
    assert FLAGS == {"interceptor": am.I_FLAGS, "vtol": am.V_FLAGS}
    for model, p in PREFIX.items():
        for b in CONTROLLER:
            assert FIX[p + "branch"][:, BRANCHES.index(b)].sum() >= 1, (model, b)
        for f in FLAGS[model]:
            assert FIX[p + "flag"][:, FLAGS[model].index(f)].sum() >= 1, (model, f)
        assert FIX[p + "ntrials"].max() <= 9 and len(FIX[p + "tf"]) <= gen.LIMIT[model]
        assert np.all(FIX[p + "tf"] <= 0.25) and np.all(FIX[p + "t0"] >= 0)
        n = FIX[p + "nrows"]
        assert all(np.all(np.isfinite(FIX[p + "states"][i][:n[i]])) and np.all(FIX[p + "B_fast"][i][:n[i]] >= 0) for i in range(len(n)))
    # t1 = PROP / Q is exact and at most 1/4 where it lies inside a segment
    two = FIX["i_phase_rows"][:, 1] > 0
    t1 = FIX["i_P"][:, am.ir.PROP] / FIX["i_P"][:, am.ir.Q]
    assert two.any() and np.all(t1[two] <= 0.25) and all(np.frexp(v)[0] == 0.5 for v in t1[two])
    # the shipped, the synthetic and the 256-obstacle table; alphaV != 0
    names = [str(m) for m in FIX["map_names"]]
    assert {"shipped", "synthetic", "grid256"} <= {names[k] for k in FIX["v_map"]}
    assert np.any(FIX["v_P"][:, am.vr.I_ALPHAV] != 0)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "adaptive_models_pin.npz")) <= 235000


@pytest.mark.parametrize("model", MODELS)
def test_float64_replay_meets_every_bound(model, capsys):
    p = PREFIX[model]
    top = {}
    for fl in ("ref", "fast"):
        for i in range(len(FIX[p + "tf"])):
            sc = gen.scenario(FIX, model, i)
            times, states, aux, r = am.emulate(sc, fl)
            n = int(FIX[p + "nrows"][i])
            assert len(times) == n and [x["accepted"] for x in r["trials"]] == list(FIX[p + "accepted"][i][:FIX[p + "ntrials"][i]] == 1.0), (fl, i)
            if model == "interceptor":
                assert np.array_equal(aux[:, 0], FIX["i_stage"][i][:n]) and np.array_equal(aux[:, 1], FIX["i_chart"][i][:n]), (fl, i)
                assert list(FIX["i_phase_rows"][i][:len(r["phase_rows"])]) == r["phase_rows"], (fl, i)
            w = worst(model, i, fl, times, states)
            top[fl] = max(top.get(fl, 0.0), w)
            assert w <= 1.0, (fl, i, w, str(FIX[p + "trail"][i]))
    with capsys.disabled():
        print("\nfloat64 replay, %s: largest err/bound %s" % (model, " ".join("%s %.3f" % kv for kv in top.items())))


def test_oracle_restatement_meets_the_reference_order_bounds(built, capsys):
    top = 0.0
    for i in range(len(FIX["i_tf"])):
        sc = gen.scenario(FIX, "interceptor", i)
        o = Oracle(MODEL_INTERCEPTOR, step_nbr=sc["step_nbr"], params=sc["P"])
        o.set_integrator(1, sc["tol"])
        Xf = o.traj(sc["t0"], sc["X0"], sc["tf"])
        r = FIX["i_nrows"][i] - 1
        w = ratios(Xf, FIX["i_states"][i][r], FIX["i_B_ref"][i][r]).max()
        top = max(top, w)
        assert w <= 1.0, (i, w, str(FIX["i_trail"][i]))
        assert o.flags()[0] == int(FIX["i_chart"][i][r])
    with capsys.disabled():
        print("\noracle, interceptor: largest end-state err/bound %.3f" % top)


@pytest.mark.parametrize("model,mutation", MUTATIONS, ids=[m for _, m in MUTATIONS])
def test_mutated_compositions_violate_a_bound_tenfold(model, mutation, capsys):
    """On the rows a mutated replay shares with the fixture.  The second figure is what the comparison at 100 x tol sees of the same
    mutated replay: |mutated - unmutated| / max(1, |unmutated|) of the end state over 100 tol, largest over scenarios (>= 1: seen)."""
    p = PREFIX[model]
    top, where, old = 0.0, None, 0.0
    for fl in ("ref", "fast"):
        for i in range(len(FIX[p + "tf"])):
            sc = gen.scenario(FIX, model, i)
            times, states, _, _ = am.emulate(sc, fl, mutation)
            w = worst(model, i, fl, times, states)
            if w > top:
                top, where = w, (fl, i)
            good = am.emulate(sc, fl)[1][-1]
            with np.errstate(all="ignore"):
                old = max(old, np.nan_to_num(np.max(np.abs(states[-1] - good) / np.maximum(1.0, np.abs(good))), nan=np.inf) / (100 * sc["tol"]))
    with capsys.disabled():
        print("\n%-17s largest err/bound %.3g at %s; against 100 x tol: %.3g (%s)" % (mutation, top, where, old, "seen" if old > 1 else "not seen"))
    assert top >= 10.0, (mutation, top)


@pytest.mark.skipif(not d5.HAVE_MPMATH, reason="the generator's arithmetic (mpmath) is not installed")
@pytest.mark.parametrize("model", MODELS)
def test_two_scenarios_regenerate_bit_for_bit(model):
    p = PREFIX[model]
    cost = FIX[p + "ntrials"].astype(float)                     # the cheapest and the median one: a 256-obstacle replay takes a minute
    if model == "vtol":
        cost = cost * np.array([len(FIX["table_" + str(FIX["map_names"][k])]) for k in FIX["v_map"]])
    by_cost = np.argsort(cost, kind="stable")
    for stored, fresh in gen.regenerate(FIX, model, [int(by_cost[0]), int(by_cost[len(by_cost) // 2])]):
        assert np.array_equal(stored, fresh, equal_nan=True)
