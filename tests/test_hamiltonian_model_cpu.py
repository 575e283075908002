"""CPU: the definition of socp_hamiltonian_gradient_batch and of a model written from its Hamiltonian alone, as
tests/hamiltonian_model_reference.py restates them.
(1) the restatement: its value part is the Hamiltonian, the H-only models' right-hand side IS the gradient; (2) width independence:
passes of 1, 2, 5 and S derivative parts give identical bits; (3) the identity G = rhs in 240 bits -- the double integrator on both
sides of the saturation, Goddard on every arc of both laws; (4) covid19: rows 4 and 6 differ by the closed forms, the other rows are
identical; (5) the instrument: three wrong restatements miss; (6) twenty RK4 steps of dint_h against the oracle's double integrator;
(7) the texts.  No GPU; the library is only asked for its symbols.

Measured (profiles/hamiltonian_model_cpu_tests.txt): |G - rhs| / max(1, |rhs|) in 240 bits is 7.4e-73 on every Goddard arc that has
a minimising law (saturated, interior and off with mu2 = 1 and 0.2; full thrust, a given singular value and off with mu2 = 0), 1.5e-72
on the closed-form singular arc AT the singular surface (Switch = 0 to 240 bits), 8.5e-73 / 0 for the double integrator.
FINDING: OFF the singular surface the closed-form singular control is a feedback, not a minimiser of H, and the identity does NOT
hold there: G - rhs = Switch (d alpha/dp, -d alpha/dx), 3.2 of the scale at the test's state (Switch = -1.38), equal to that closed form
to 1.2e-73.  The reference integrates that arc only where Switch = 0 holds to solver tolerance; a model written from H alone would
leave it at the rate Switch grad alpha.  covid19: rows 4 and 6 miss by 4.4e-4 ... of the scale, exactly the closed forms."""
import os

import numpy as np
import pytest

import fast_reference as fa
import fields_reference as fr
import hamiltonian_model_reference as hm
from fields_reference import mpf, mpmath
from test_fields_cpu import X0_GODDARD, X0_DINT, X0_DINT_SAT, goddard_rows, dint_oracle, covid_oracle, oracle_trajectory

pytestmark = pytest.mark.skipif(not fr.HAVE_MPMATH, reason="mpmath is the 240-bit carrier")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = mpf(2) ** -200 if fr.HAVE_MPMATH else None
GODDARD_P = [3.5, 7.0, 310.0, 500.0, 1.0, 1.0, 1.0, -1.0]          # C, b, KD, kr, u_max, mu1, mu2, singularControl
DINT_P = [1.0, 1.0, 0.01]
COVID_P = [3.4, 14.0, 5.0, 1.0, 0.1, 1.0, 0.0, 0.8]                # R0, Tinf, Tinc, N, Imax, muI, umin, umax
SW = (0.05, 0.15)


def record(key, line):
    """The figures of a run (pytest -s): profiles/hamiltonian_model_cpu_tests.txt keeps the lines of the run on record."""
    print("[hamiltonian_model_cpu %s] %s" % (key, line))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def norm(v):
    return max(abs(q) for q in v)


def goddard_state(p_mass=None):
    X = X0_GODDARD.copy()
    X[3:6] = [0.01, 0.02, -0.015]
    if p_mass is not None:
        X[13] = p_mass
    return X


def goddard_params(mu2, sing=-1.0):
    P = list(GODDARD_P)
    P[6], P[7] = mu2, sing
    return P


def covid_state(clamp, above):
    """clamp: "min" (u <= umin), "max" (u >= umax) or None; above: I >= Imax."""
    pS, pE = {"min": (1.0, -1.0), "max": (-300.0, 100.0), None: (-10.0, 10.0)}[clamp]
    return np.array([0.8, 0.05, 0.15 if above else 0.05, 0.1, pS, pE, 0.3, -0.2])


def points(model, count=40, seed=31):
    """(P, sw, t[count], X[count][S]) with every branch of the model's law among them."""
    rng = np.random.default_rng(seed)
    if model.startswith("goddard"):
        mu2 = {"goddard mu2=1": 1.0, "goddard mu2=0.2": 0.2, "goddard mu2=0": 0.0}[model]
        X, t = goddard_rows(rng, count, SW)
        X[:, 13] *= rng.choice([-10.0, 0.5, 1.0, 4.0], size=count)
        return "goddard", goddard_params(mu2), SW, t, X
    if model == "dint":
        X = rng.uniform(-1.0, 1.0, size=(count, 12)) * rng.choice([0.3, 3.0], size=(count, 1))
        return "dint", DINT_P, (0.0, 0.0), np.zeros(count), X
    if model == "covid":
        X = np.array([covid_state(c, a) for c in ("min", "max", None) for a in (False, True)] * ((count + 5) // 6))[:count]
        X = X * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, size=X.shape))
        return "covid", COVID_P, (0.0, 0.0), np.zeros(count), X
    X = rng.uniform(0.2, 1.0, size=(count, 2)) * rng.choice([-1.0, 1.0], size=(count, 2))
    return "osc1d", [4.0], (0.0, 0.0), np.zeros(count), X


ALL_MODELS = ["goddard mu2=1", "goddard mu2=0.2", "goddard mu2=0", "dint", "covid", "osc1d"]


# ---- (1) the restatement ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL_MODELS)
def test_1_the_value_part_is_the_hamiltonian_and_the_seeds_are_read(name):
    model, P, sw, t, X = points(name, count=12)
    for k in range(len(X)):
        S = len(X[k])
        Y = [fr.Dual(float(X[k][i]), np.array([1.0 if i == c else 0.0 for c in range(S)])) for i in range(S)]
        with np.errstate(all="ignore"):
            H = hm.HAMILTONIAN[model](fr.DualKit(), [float(p) for p in P], list(sw), float(t[k]), Y)
        assert bits(H.v) == bits(hm.plain_hamiltonian(model, P, sw, t[k], X[k])), k
        G = hm.symplectic_gradient(model, P, sw, t[k], X[k])
        D = S // 2
        assert np.array_equal(bits(G[:D]), bits(H.d[D:])) and np.array_equal(bits(G[D:]), bits(-H.d[:D])), k


def test_1_the_h_only_models_right_hand_side_is_the_gradient():
    for name, base in hm.BASE.items():
        model, P, sw, t, X = points(base, count=8)
        for k in range(len(X)):
            assert np.array_equal(bits(hm.plain_rhs(name, P, sw, t[k], X[k])), bits(hm.symplectic_gradient(base, P, sw, t[k], X[k])))
            assert bits(hm.plain_hamiltonian(name, P, sw, t[k], X[k])) == bits(hm.plain_hamiltonian(base, P, sw, t[k], X[k]))
    assert set(hm.BASE) <= set(hm.RHS) and not set(hm.BASE) & set(fr.RHS), "the entries live in the helper's table only"


def test_1_the_lent_entries_are_taken_back():
    import exact_jacobian_reference as ejr
    with hm.entries():
        assert "dint_h" in ejr.RHS and "dint_h" in ejr.HAMILTONIAN
    assert not set(hm.BASE) & (set(ejr.RHS) | set(ejr.HAMILTONIAN) | set(ejr.SWITCHING_READS_XP))


# ---- (2) width independence -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL_MODELS)
def test_2_every_pass_width_gives_the_same_bits(name):
    model, P, sw, t, X = points(name)
    S = X.shape[1]
    whole = hm.gradient_batch(model, P, t, X, sw=[sw] * len(X))
    assert np.all(np.isfinite(whole))
    for W in sorted({1, min(2, S), min(5, S), S}):
        cut = hm.gradient_batch(model, P, t, X, sw=[sw] * len(X), width=W)
        assert np.array_equal(bits(whole), bits(cut)), W


# ---- (3) the identity in 240 bits -------------------------------------------------------------------------------------------------

def identity(model, P, sw, t, X):
    """(|G - rhs|, max(1, |rhs|)) in 240 bits."""
    G = hm.symplectic_gradient(model, P, sw, t, X, high=True)
    R = hm.rhs_high(model, P, sw, t, X)
    return norm([g - r for g, r in zip(G, R)]), max(mpf(1), norm(R))


@pytest.mark.parametrize("X0, saturated", [(X0_DINT, False), (X0_DINT_SAT, True)])
def test_3_double_integrator_on_both_sides_of_the_saturation(X0, saturated):
    u = -X0[9:12] / DINT_P[1]
    assert (np.sqrt(u @ u) > DINT_P[0]) == saturated
    d, scale = identity("dint", DINT_P, (0.0, 0.0), 0.0, X0)
    record("identity", "dint saturated=%s  |G - rhs| / max(1, |rhs|) = %.3e" % (saturated, float(d / scale)))
    assert d <= BAR * scale


def goddard_switch(P, X):
    return P[5] - P[1] * X[13] - P[0] / X[6] * np.sqrt(X[10] ** 2 + X[11] ** 2 + X[12] ** 2)


GODDARD_ARCS = {        # name: (mu2, singularControl, t, p_mass, the arc's condition on alpha = -Switch / 2 / mu2 or on t)
    "smooth mu2=1 saturated": (1.0, -1.0, 0.0, 0.2, lambda a: a > 1.0),
    "smooth mu2=1 interior": (1.0, -1.0, 0.0, 0.05, lambda a: 0.0 < a < 1.0),
    "smooth mu2=1 off": (1.0, -1.0, 0.0, -2.0, lambda a: a <= 0.0),
    "smooth mu2=0.2 saturated": (0.2, -1.0, 0.0, None, lambda a: a > 1.0),
    "smooth mu2=0.2 interior": (0.2, -1.0, 0.0, -0.08, lambda a: 0.0 < a < 1.0),
    "smooth mu2=0.2 off": (0.2, -1.0, 0.0, -2.0, lambda a: a <= 0.0),
    "general full thrust": (0.0, -1.0, 0.02, None, None),
    "general given singular value": (0.0, 0.6, 0.1, None, None),
    "general off": (0.0, -1.0, 0.18, None, None),
}


@pytest.mark.parametrize("arc", list(GODDARD_ARCS))
def test_3_goddard_on_every_arc_with_a_minimising_law(arc):
    mu2, sing, t, p_mass, cond = GODDARD_ARCS[arc]
    P, X = goddard_params(mu2, sing), goddard_state(p_mass)
    if cond is not None:
        assert cond(-goddard_switch(P, X) / 2 / mu2), "the state is on the arc it is named for"
    else:
        assert (t <= SW[0]) == ("full" in arc) and (t > SW[1]) == ("off" in arc)
    d, scale = identity("goddard", P, SW, t, X)
    record("identity", "goddard %-30s |G - rhs| / max(1, |rhs|) = %.3e" % (arc, float(d / scale)))
    assert d <= BAR * scale


def singular_alpha(P, X):
    """The closed-form singular thrust as a 240-bit dual number with 14 derivative parts, its value, and Switch."""
    K = fr.DualMpfKit()
    num = lambda q: q if isinstance(q, mpmath.mpf) else mpf(float(q))                     # noqa: E731
    Pn = [num(p) for p in P]
    Y = [fr.DualMpf(num(X[i]), np.array([mpf(1.0) if i == k else mpf(0.0) for k in range(14)], dtype=object)) for i in range(14)]
    x, y, z, vx, vy, vz, mass = Y[0:7]
    p_vx, p_vy, p_vz = Y[10:13]
    r = K.sqrt(x*x + y*y + z*z)
    v = K.sqrt(vx*vx + vy*vy + vz*vz)
    pvdotv = p_vx*vx + p_vy*vy + p_vz*vz
    norm_pv = K.sqrt(p_vx*p_vx + p_vy*p_vy + p_vz*p_vz)
    a = fa._singular(K, Pn, Y, r, v, 1 / r / r, norm_pv, K.exp(-Pn[3]*(r - 1)), pvdotv)
    return a, (Pn[5] - Pn[1]*Y[13] - Pn[0] / mass*norm_pv).v


def test_3_goddard_singular_arc_on_the_singular_surface():
    """The closed-form singular control where it belongs: p_mass set in 240 bits so that Switch = 0."""
    P = goddard_params(0.0, -1.0)
    X = [mpf(float(q)) for q in goddard_state()]
    X[13] = (mpf(P[5]) - mpf(P[0]) / X[6] * mpmath.sqrt(X[10] ** 2 + X[11] ** 2 + X[12] ** 2)) / mpf(P[1])
    a, switch = singular_alpha(P, X)
    assert abs(switch) <= mpf(2) ** -230 and 0 < a.v < P[4], "on the surface, thrust inside its bounds"
    d, scale = identity("goddard", P, SW, 0.1, X)
    record("identity", "goddard %-30s |G - rhs| / max(1, |rhs|) = %.3e  (alpha = %.4f)" % ("general singular arc, Switch = 0", float(d / scale), float(a.v)))
    assert d <= BAR * scale


def test_3_finding_off_the_singular_surface_the_closed_form_control_is_no_minimiser():
    """FINDING, pinned: with Switch != 0 the singular feedback does not minimise H, and the total derivative carries
    Switch * grad alpha:  G - rhs = Switch (d alpha/dp, -d alpha/dx), in 240 bits."""
    P, X = goddard_params(0.0, -1.0), goddard_state()
    a, switch = singular_alpha(P, X)
    assert 0 < a.v < P[4] and abs(switch) > 1
    G = hm.symplectic_gradient("goddard", P, SW, 0.1, X, high=True)
    R = hm.rhs_high("goddard", P, SW, 0.1, X)
    diff = [g - r for g, r in zip(G, R)]
    want = [switch * a.d[i + 7] for i in range(7)] + [-(switch * a.d[i]) for i in range(7)]
    miss = norm([d - w for d, w in zip(diff, want)])
    record("finding", "goddard singular arc off the surface: Switch = %.4f, alpha = %.4f, |G - rhs| / max(1, |rhs|) = %.3e; against "
           "Switch (d alpha/dp, -d alpha/dx): %.3e of |G - rhs|" % (float(switch), float(a.v), float(norm(diff) / max(1, norm(R))), float(miss / norm(diff))))
    assert norm(diff) > mpf(10) ** -3 * max(1, norm(R)), "the identity does not hold here"
    assert miss <= BAR * norm(diff)


# ---- (4) covid19: an upstream property, kept for parity -------------------------------------------------------------------------

@pytest.mark.parametrize("clamp", ["min", "max", None])
@pytest.mark.parametrize("above", [False, True])
def test_4_covid_rows_4_and_6_differ_by_the_closed_forms(clamp, above):
    P, X = COVID_P, covid_state(clamp, above)
    u_free = (X[5] - X[4]) * X[0] * X[2] / P[1] / P[3] * P[0]
    assert {"min": u_free <= P[6], "max": u_free >= P[7], None: P[6] < u_free < P[7]}[clamp] and (X[2] >= P[4]) == above
    G = hm.symplectic_gradient("covid", P, (0.0, 0.0), 0.0, X, high=True)
    R = hm.rhs_high("covid", P, (0.0, 0.0), 0.0, X)
    scale = max(mpf(1), norm(R))
    for row in (0, 1, 2, 3, 5, 7):
        # a clamped control is a constant: the same 240-bit numbers.  An unclamped one brings dH/du du/dX = (u - u') du/dX, with u'
        # the same control formed in another order: zero to the rounding of 240 bits, not exactly (2.3e-75 at this state)
        assert (G[row] == R[row]) if clamp else (abs(G[row] - R[row]) <= BAR * scale), row
    Sx, I, Rx, pS, pE = (mpf(float(X[k])) for k in (0, 2, 3, 4, 5))
    R0, Tinf, N = mpf(P[0]), mpf(P[1]), mpf(P[3])
    u = mpf(float({"min": P[6], "max": P[7]}[clamp])) if clamp else (pE - pS) * Sx * I / Tinf / N * R0
    Rt = R0 * (1 - u)
    want = {4: (pS - pE) * (Rt - Rx) * I / Tinf / N, 6: (pS - pE) * (Rt - Rx) * Sx / Tinf / N}
    for row in (4, 6):
        assert abs(want[row]) > mpf(10) ** -6, "the rows do differ"
        assert abs((G[row] - R[row]) - want[row]) <= BAR * scale, row
    record("covid19", "clamp=%-4s I>=Imax=%-5s G - rhs rows 4, 6 = %.3e, %.3e  (%.3e of the scale)"
           % (clamp, above, float(G[4] - R[4]), float(G[6] - R[6]), float(max(abs(G[4] - R[4]), abs(G[6] - R[6])) / scale)))


def test_4_the_restated_covid_dynamics_are_the_upstream_text():
    """What rows 4 and 6 are compared with is the oracle's right-hand side, bit for bit, R = X[3] included."""
    o = covid_oracle()
    P = o.params()[:8]
    for clamp in ("min", "max", None):
        X = covid_state(clamp, True)
        assert np.array_equal(bits(o.rhs(0.0, X)), bits(hm.plain_rhs("covid", P, (0.0, 0.0), 0.0, X)))


# ---- (5) the instrument -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mutate", hm.MUTATIONS)
@pytest.mark.parametrize("name", ALL_MODELS)
def test_5_wrong_restatements_miss_the_gradient(name, mutate):
    model, P, sw, t, X = points(name, count=1)
    if model == "goddard":
        X = [goddard_state()]
    G = hm.symplectic_gradient(model, P, sw, 0.1, X[0], high=True)
    Gm = hm.symplectic_gradient(model, P, sw, 0.1, X[0], high=True, mutate=mutate)
    miss = norm([a - b for a, b in zip(G, Gm)]) / norm(G)
    record("instrument", "%-16s %-12s off by %.3e of the gradient's scale" % (name, mutate, float(miss)))
    assert miss > mpf(10) ** -3


# ---- (6) dint_h along a trajectory ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("X0, label", [(X0_DINT, "unsaturated"), (X0_DINT_SAT, "saturated")])
def test_6_twenty_steps_of_dint_h_against_the_oracle_trajectory(X0, label):
    N, t2 = 20, 3.0
    o = dint_oracle(N)
    P = o.params()[:3]
    ref = np.array(oracle_trajectory(o, 0.0, t2, X0, N))
    own = np.array(hm.integrate("dint_h", P, (0.0, 0.0), 0.0, t2, X0, N))
    assert ref.shape == own.shape == (N, 12)
    truth_h = hm.integrate("dint_h", P, (0.0, 0.0), 0.0, t2, X0, N, high=True)
    truth_o = hm.integrate("dint", P, (0.0, 0.0), 0.0, t2, X0, N, high=True)
    dev = lambda A, T: max(abs(mpf(float(A[k][j])) - T[k][j]) for k in range(N) for j in range(12))       # noqa: E731
    dev_h, dev_o = dev(own, truth_h), dev(ref, truth_o)
    gap = float(np.max(np.abs(own - ref)))
    allowed = 8 * (dev_h + dev_o)
    record("trajectory", "dint_h %-11s 20 steps: |X_h - X_oracle| = %.3e, own deviations %.3e + %.3e, ratio to the allowance %.3f"
           % (label, gap, float(dev_h), float(dev_o), float(gap / allowed) if allowed else 0.0))
    assert gap <= allowed


# ---- (7) the texts ----------------------------------------------------------------------------------------------------------------

def test_7_abi_plugins_and_symbols():
    launch = open(os.path.join(ROOT, "socp_amd", "csrc", "launch.hpp")).read()
    assert "kPluginAbi = 16" in launch and "kPluginAbi = 15:" in launch
    for name in ("osc1d_h_plugin.hip", "dint_h_plugin.hip"):
        text = open(os.path.join(ROOT, "tests", "plugin", name)).read()
        assert "SOCP_DEFINE_HAMILTONIAN_PLUGIN" in text and "hamiltonian_t" in text
        assert " rhs(" not in text and "rhs_t" not in text, "no hand-written dynamics"
    import ctypes
    from socp_amd import capi
    lib = ctypes.CDLL(capi.LIB_PATH)
    for sym in ("socp_ctx_has_hamiltonian_gradient", "socp_hamiltonian_gradient_batch_dev", "socp_hamiltonian_gradient_batch"):
        assert hasattr(lib, sym), sym
    header = open(os.path.join(ROOT, "include", "socp_hip.h")).read()
    assert "HAMILTONIAN GRADIENT" in header and "covid19.cpp:88,90" in header
