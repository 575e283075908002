"""CPU: the instrument that pins the adaptive Dormand-Prince integrator (tests/dopri5_reference.py, tests/golden/dopri5_pin.npz)
is itself checked before any kernel is judged by it.

  * the tableau the replay runs on is the published pair: order conditions in exact rational arithmetic, and SciPy's own copy;
  * the replay in numpy.float64 meets every bound of the fixture (the error model covers a correct implementation);
  * nine deliberately wrong float64 replays (dopri5_reference.MUTATIONS: a wrong error weight, a stage coefficient off by 1e-9,
    the norm on the wrong state or without h |k1|, and five changes of the controller) each VIOLATE a bound of at least one
    scenario BY A FACTOR >= 10: the bounds are tight enough to be worth having.  That factor is a condition on the fixture;
  * the CPU oracle's restatement (oracle/socp_oracle.c: orc_integrate_dopri5, orc_integrate_dopri5_jac) meets the reference-order
    bounds on every scenario and reports the fixture's accepted and rejected counts exactly;
  * with mpmath present, two scenarios per model evaluated afresh equal the stored fixture bit for bit."""
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest

import dopri5_reference as d5
from oracle.oracle import Oracle, MODEL_GODDARD, MODEL_COVID, MODEL_DINT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "dopri5_pin.npz"))
PREFIX = {"goddard": "g_", "covid": "c_", "dint": "d_", "dint_aug": "a_"}
ORACLE_ID = {"goddard": MODEL_GODDARD, "covid": MODEL_COVID, "dint": MODEL_DINT, "dint_aug": MODEL_DINT}
MODELS = list(PREFIX)
BRANCHES = [str(b) for b in FIX["branch_names"]]
TABLE = ["single_cap", "grow", "keep", "reject", "clamp", "reject2", "reinit", "kink"]
QUOTA = {"goddard": 4, "covid": 1, "dint": 2, "dint_aug": 2}


def scenario(model, i):
    p = PREFIX[model]
    return dict(model=model, P=[float(v) for v in FIX[p + "P"][i]], sw=[float(v) for v in FIX[p + "sw"][i]], tol=float(FIX[p + "tol"][i]),
                tf=float(FIX[p + "tf"][i]), step_nbr=int(FIX[p + "step_nbr"][i]), X0=FIX[p + "X0"][i])


def ratios(got, val, B):
    """|got - val| / B per component, 0 where both vanish (a bound of zero demands equality)."""
    err = np.abs(got - val)
    with np.errstate(all="ignore"):
        return np.where(err == 0, 0.0, err / B)


def worst(model, i, fl, times, states):
    """The largest |got - value| / bound over the rows a replay shares with the fixture (times and states)."""
    p = PREFIX[model]
    r = min(len(times), int(FIX[p + "nrows"][i]))
    rt = ratios(times[:r], FIX[p + "times"][i][:r], FIX[p + "Bt_" + fl][i][:r])
    rs = ratios(states[:r], FIX[p + "states"][i][:r], FIX[p + "B_" + fl][i][:r])
    return max(np.nan_to_num(rt, nan=np.inf).max(), np.nan_to_num(rs, nan=np.inf).max())


# ---- the tableau ---------------------------------------------------------------------------------------------------------------

def _order_conditions(b):
    """Residuals of the 17 order conditions of a 7-stage explicit method with weights b (Butcher; Hairer, Norsett & Wanner II.2),
    grouped by order, in exact rational arithmetic."""
    s = 7
    A = [[d5.STAGES[i][j] if j < len(d5.STAGES[i]) else Fr(0) for j in range(s)] for i in range(s)]
    c = d5.NODES
    mv = lambda v: [sum(A[i][j] * v[j] for j in range(s)) for i in range(s)]          # A v
    had = lambda u, v: [x * y for x, y in zip(u, v)]
    pw = lambda v, k: [x ** k for x in v]
    dot = lambda v: sum(x * y for x, y in zip(b, v))
    one = [Fr(1)] * s
    Ac, Ac2, Ac3 = mv(c), mv(pw(c, 2)), mv(pw(c, 3))
    AAc = mv(Ac)
    return {
        1: [dot(one) - 1],
        2: [dot(c) - Fr(1, 2)],
        3: [dot(pw(c, 2)) - Fr(1, 3), dot(Ac) - Fr(1, 6)],
        4: [dot(pw(c, 3)) - Fr(1, 4), dot(had(c, Ac)) - Fr(1, 8), dot(Ac2) - Fr(1, 12), dot(AAc) - Fr(1, 24)],
        5: [dot(pw(c, 4)) - Fr(1, 5), dot(had(pw(c, 2), Ac)) - Fr(1, 10), dot(had(Ac, Ac)) - Fr(1, 20), dot(had(c, Ac2)) - Fr(1, 15),
            dot(Ac3) - Fr(1, 20), dot(had(c, AAc)) - Fr(1, 30), dot(mv(had(c, Ac))) - Fr(1, 40), dot(mv(Ac2)) - Fr(1, 60),
            dot(mv(AAc)) - Fr(1, 120)],
    }


def test_tableau_satisfies_the_order_conditions_exactly():
    for i, row in enumerate(d5.STAGES):
        assert sum(row, Fr(0)) == d5.NODES[i], i                                    # row sums are the nodes
    assert d5.STAGES[6] + [Fr(0)] == d5.B5                                          # FSAL: the last stage is the new state
    r5, r4 = _order_conditions(d5.B5), _order_conditions(d5.B4)
    assert all(v == 0 for k in range(1, 6) for v in r5[k])                          # fifth order
    assert all(v == 0 for k in range(1, 5) for v in r4[k])                          # fourth order ...
    assert any(v != 0 for v in r4[5])                                               # ... and not fifth
    assert sum(len(v) for v in r5.values()) == 17


def test_tableau_is_scipys():
    """An independent carrier of the same published table: scipy.integrate.RK45 (E = fourth-order minus fifth-order weights)."""
    pytest.importorskip("scipy")
    from scipy.integrate import RK45
    f = lambda v: np.array([float(x) for x in v])
    assert np.allclose(RK45.C, f(d5.NODES[:6]), rtol=2e-16, atol=0)
    for i in range(6):
        assert np.allclose(RK45.A[i, :i], f(d5.STAGES[i]), rtol=2e-16, atol=0), i
        assert not RK45.A[i, i:].any()
    assert np.allclose(RK45.B, f(d5.B5[:6]), rtol=2e-16, atol=0)
    E = [b4 - b5 for b4, b5 in zip(d5.B4, d5.B5)]
    assert np.allclose(RK45.E, f(E), rtol=4e-16, atol=0) and RK45.E[1] == 0


# ---- the fixture ---------------------------------------------------------------------------------------------------------------

def test_fixture_fills_the_branch_table_with_decidable_scenarios():
    """Every row of the controller's branch table at its minimum, per model (and so per flavour: a scenario is kept only if it is
    decidable in every flavour of its model); short segments; tf <= 1/4; C_POW and DECIDE_FACTOR as the helper has them."""
    assert int(FIX["c_pow"]) == d5.C_POW and int(FIX["decide_factor"]) == d5.DECIDE_FACTOR and BRANCHES == d5.BRANCHES
    for model, p in PREFIX.items():
        table = FIX[p + "branch"][FIX[p + "group"] == 0]
        for b in TABLE:
            assert table[:, BRANCHES.index(b)].sum() >= QUOTA[model], (model, b)
        assert table[:, BRANCHES.index("reinit_reject")].sum() >= 1 and table[:, BRANCHES.index("grow_04")].sum() >= 1, model
        assert FIX[p + "ntrials"].max() <= 9 and FIX[p + "tf"].max() <= 0.25 and FIX[p + "step_nbr"].max() <= 4
        assert np.all((FIX[p + "tol"] >= 1e-6) & (FIX[p + "tol"] <= 1e-3))
        assert np.array_equal(FIX[p + "nrows"], FIX[p + "n_accepted"] + 1)
    # Goddard's kink scenarios include the bang / singular / off law (mu2 = 0); the augmented scenarios start saturated
    kink = FIX["g_branch"][:, BRANCHES.index("kink")]
    assert np.sum(kink & (FIX["g_P"][:, 6] == 0.0)) >= 1
    assert np.all(np.linalg.norm(FIX["a_X0"][:, 9:12], axis=1) / FIX["a_P"][:, 1] > FIX["a_P"][:, 0])
    assert set(FIX["a_group"]) == {0, 1, 2}


@pytest.mark.parametrize("model", MODELS)
def test_float64_replay_meets_every_bound(model, capsys):
    p = PREFIX[model]
    top = {}
    for fl in d5.FLAVOURS[model]:
        for i in range(len(FIX[p + "tf"])):
            s = scenario(model, i)
            times, states, acc, rej = d5.emulate(model, fl, s["P"], s["sw"], s["tol"], s["tf"], s["step_nbr"], s["X0"])
            assert len(times) == FIX[p + "nrows"][i] and (acc, rej) == (FIX[p + "n_accepted"][i], FIX[p + "n_rejected"][i]), (fl, i)
            w = worst(model, i, fl, times, states)
            top[fl] = max(top.get(fl, 0.0), w)
            assert w <= 1.0, (fl, i, w, str(FIX[p + "trail"][i]))
    with capsys.disabled():
        print("\nfloat64 replay, %s: largest err/bound %s" % (model, " ".join("%s %.3f" % kv for kv in top.items())))


@pytest.mark.parametrize("mutation", list(d5.MUTATIONS))
def test_mutated_replays_violate_a_bound_tenfold(mutation, capsys):
    """On the rows a mutated replay shares with the fixture (a mutation that changes a step size changes every later time)."""
    top, where = 0.0, None
    for model, p in PREFIX.items():
        for fl in d5.FLAVOURS[model]:
            for i in range(len(FIX[p + "tf"])):
                s = scenario(model, i)
                with np.errstate(all="ignore"):
                    r = d5.replay(d5.D5F64(), model, fl, s["P"], s["sw"], s["tol"], s["tf"], s["step_nbr"], s["X0"], mut=mutation)
                w = worst(model, i, fl, np.array(r["times"], dtype=float), np.array(r["states"], dtype=float))
                if w > top:
                    top, where = w, (model, fl, i)
    with capsys.disabled():
        print("\n%-13s largest err/bound %.3g at %s" % (mutation, top, where))
    assert top >= 10.0, (mutation, top)


@pytest.mark.parametrize("model", MODELS)
def test_oracle_restatement_meets_the_reference_order_bounds(built, model, capsys):
    p = PREFIX[model]
    top = 0.0
    for i in range(len(FIX[p + "tf"])):
        s = scenario(model, i)
        o = Oracle(ORACLE_ID[model], step_nbr=s["step_nbr"], params=s["P"])
        o.set_switching(s["sw"])
        Xf, acc, rej = o.traj_dopri5(0.0, s["X0"], s["tf"], s["tol"], is_jac=int(model == "dint_aug"))
        assert (acc, rej) == (FIX[p + "n_accepted"][i], FIX[p + "n_rejected"][i]), (i, str(FIX[p + "trail"][i]))
        r = FIX[p + "nrows"][i] - 1
        w = ratios(Xf, FIX[p + "states"][i][r], FIX[p + "B_ref"][i][r]).max()
        top = max(top, w)
        assert w <= 1.0, (i, w, str(FIX[p + "trail"][i]))
    with capsys.disabled():
        print("\noracle, %s: largest end-state err/bound %.3f" % (model, top))


@pytest.mark.skipif(not d5.HAVE_MPMATH, reason="the generator's arithmetic (mpmath) is not installed")
@pytest.mark.parametrize("model", MODELS)
def test_two_scenarios_regenerate_bit_for_bit(model):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_dopri5_golden as gen
    finally:
        sys.path.pop(0)
    n = len(FIX[PREFIX[model] + "tf"])
    for stored, fresh in gen.regenerate(FIX, model, [0, n - 1]):
        assert np.array_equal(stored, fresh, equal_nan=True)
