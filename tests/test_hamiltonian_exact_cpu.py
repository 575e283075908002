"""CPU: NESTED DUAL NUMBERS, socp_hamiltonian_jacobian_batch and the exact H-only models (plugin::FromHamiltonianExact), as
tests/hamiltonian_exact_reference.py restates them.
(1) width independence of the nested gradient, its value parts the gradient's bits; (2) A against 240-bit central differences of the
240-bit gradient; (3) -Omega A symmetric in 240 bits on every point strictly inside a branch; (4) A against d rhs_t/dX of the
hand-written texts where G = rhs on an open set, and NOT equal on Goddard's closed-form singular arc and for covid19; (5) doubles
against their own 240-bit truth; (6) dint_hx and the in-tree double integrator are the same problem: exact Jacobian and Phi; (7) the
four wrong restatements miss; (8) texts and symbols.  No GPU; the library is only asked for its symbols.
The figures a run prints (pytest -s) are kept in profiles/hamiltonian_exact_cpu_tests.txt."""
import os

import numpy as np
import pytest

import exact_jacobian_reference as ejr
import fields_reference as fr
import hamiltonian_exact_reference as hx
import hamiltonian_model_reference as hm
import sensitivity_reference as sr
import test_hamiltonian_model_cpu as cpu
from fields_reference import mpf
from test_fields_cpu import X0_DINT, X0_DINT_SAT

pytestmark = pytest.mark.skipif(not fr.HAVE_MPMATH, reason="mpmath is the 240-bit carrier")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = cpu.BAR                                   # 2^-200: the bar of the gradient check
H80 = mpf(2) ** -80 if fr.HAVE_MPMATH else None  # the step of test_exact_jacobian_cpu.py's 240-bit central differences
TOL_FD = 1e-40                                  # and their bar: truncation h^2 / 6 |G'''| with h^2 = 6.8e-49, rounding 2^-240 / h = 7e-49
DINT_P, SW = cpu.DINT_P, cpu.SW
bits, norm = cpu.bits, cpu.norm


def record(key, line):
    print("[hamiltonian_exact_cpu %s] %s" % (key, line))


def amax(A):
    return max(abs(q) for q in np.asarray(A).ravel())


def omega_t_a(A):
    """-Omega A = the Hessian: rows D .. S-1 of A negated on top, rows 0 .. D-1 below (Omega = [0 I; -I 0])."""
    S = A.shape[0]
    D = S // 2
    return np.array([[-A[i + D, j] for j in range(S)] for i in range(D)] + [[A[i, j] for j in range(S)] for i in range(D)], dtype=object)


# the points strictly inside a branch (test_hamiltonian_model_cpu.py's): name -> (model, P, sw, t, X, G == rhs on an open set)
def inside_points():
    out = {"dint unsaturated": ("dint", DINT_P, (0.0, 0.0), 0.0, X0_DINT, True), "dint saturated": ("dint", DINT_P, (0.0, 0.0), 0.0, X0_DINT_SAT, True)}
    for arc, (mu2, sing, t, p_mass, _) in cpu.GODDARD_ARCS.items():
        out["goddard " + arc] = ("goddard", cpu.goddard_params(mu2, sing), SW, t, cpu.goddard_state(p_mass), True)
    out["goddard general closed-form singular arc"] = ("goddard", cpu.goddard_params(0.0, -1.0), SW, 0.1, cpu.goddard_state(), False)
    for clamp in ("min", "max", None):
        for above in (False, True):
            out["covid clamp=%s above=%s" % (clamp, above)] = ("covid", cpu.COVID_P, (0.0, 0.0), 0.0, cpu.covid_state(clamp, above), False)
    out["osc1d"] = ("osc1d", [4.0], (0.0, 0.0), 0.0, np.array([0.7, -0.4]), True)
    return out


INSIDE = inside_points()
_A240 = {}


def a240(name):
    if name not in _A240:
        model, P, sw, t, X, _ = INSIDE[name]
        _A240[name] = hx.hamiltonian_jacobian(model, P, sw, t, X, high=True)
    return _A240[name]


# ---- (1) width does not matter ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cpu.ALL_MODELS)
def test_1_every_inner_width_gives_the_same_bits_and_the_value_parts_are_the_gradient(name):
    model, P, sw, t, X = cpu.points(name, count=20)
    S = X.shape[1]
    for k in range(len(X)):
        A, G = hx.hamiltonian_jacobian(model, P, sw, t[k], X[k], width=S)
        assert np.all(np.isfinite(A))
        for W in (1, min(2, S)):
            Aw, Gw = hx.hamiltonian_jacobian(model, P, sw, t[k], X[k], width=W)
            assert np.array_equal(bits(A), bits(Aw)) and np.array_equal(bits(G), bits(Gw)), (k, W)
        assert np.array_equal(bits(G), bits(np.array(hm.symplectic_gradient(model, P, sw, t[k], X[k])))), "the value parts are the gradient"


# ---- (2) the matrix is right, in 240 bits --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(INSIDE))
def test_2_the_matrix_against_central_differences_of_the_240_bit_gradient(name):
    model, P, sw, t, X, _ = INSIDE[name]
    A, G = a240(name)
    S = len(X)
    worst = mpf(0)
    for j in range(S):
        sides = []
        for sgn in (1, -1):
            Xm = [mpf(float(x)) for x in X]
            Xm[j] = Xm[j] + sgn * H80
            sides.append(hm.symplectic_gradient(model, P, sw, t, Xm, high=True))
        worst = max(worst, max(abs(A[i, j] - (a - b) / (2 * H80)) for i, (a, b) in enumerate(zip(*sides))))
    scale = max(mpf(1), amax(A))
    record("2", "%-42s |A - central differences (step 2^-80)| / max(1, |A|) = %.3e   (|A| = %.3e)" % (name, float(worst / scale), float(amax(A))))
    assert worst <= TOL_FD * scale


# ---- (3) symmetry ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(INSIDE))
def test_3_minus_omega_a_is_symmetric(name):
    A, _ = a240(name)
    Hs = omega_t_a(A)
    S = A.shape[0]
    asym = max(abs(Hs[i, j] - Hs[j, i]) for i in range(S) for j in range(S))
    scale = max(mpf(1), amax(A))
    record("3", "%-42s |(-Omega A) - (-Omega A)^T| / max(1, |A|) = %.3e" % (name, float(asym / scale)))
    assert asym <= BAR * scale


# ---- (4) A against the hand-written texts ---------------------------------------------------------------------------------------------

def drhs_240(model, P, sw, t, X):
    """d rhs_t / dX in 240 bits: fr.RHS on DualMpfKit with unit seeds."""
    S = len(X)
    Y = [fr.DualMpf(mpf(float(X[i])), np.array([mpf(1.0) if i == j else mpf(0.0) for j in range(S)], dtype=object)) for i in range(S)]
    zero = np.array([mpf(0.0)] * S, dtype=object)
    with np.errstate(all="ignore"):
        R = fr.rhs_on(fr.RHS[model], fr.DualMpfKit(), [mpf(float(p)) for p in P], [mpf(float(s)) for s in sw], mpf(float(t)), Y)
    return np.array([(r.d if isinstance(r, fr.Dual) else zero) for r in R], dtype=object)


@pytest.mark.parametrize("name", [n for n in INSIDE if n != "osc1d"])
def test_4_the_matrix_against_the_hand_written_right_hand_side(name):
    model, P, sw, t, X, agrees = INSIDE[name]
    A, _ = a240(name)
    J = drhs_240(model, P, sw, t, X)
    diff = amax(A - J)
    scale = max(mpf(1), amax(J))
    record("4", "%-42s |A - d rhs_t/dX| / max(1, |d rhs_t/dX|) = %.3e  (%s)" % (name, float(diff / scale), "asserted equal" if agrees else "FINDING: not equal"))
    if agrees:
        assert diff <= BAR * scale
    else:
        assert diff > BAR * scale, "G is not rhs here, or agrees on a surface only: A is not its Jacobian"


# ---- (5) doubles against their own truth -----------------------------------------------------------------------------------------------

def dint_hx_cases():
    """name -> (prob, z, N): M = 1, N = 20 unsaturated and saturated; M = 3 with a free interior time and a free final time."""
    from oracle.oracle import Problem, FIXED, FREE, CONTINUOUS
    out = {}
    for label, X0 in (("unsaturated", X0_DINT), ("saturated", X0_DINT_SAT)):
        mode_x = np.zeros((2, 6), dtype=np.int32)
        mode_x[1, 3:] = FREE
        xn = np.zeros((2, 12))
        xn[0, :6] = X0[:6]
        xn[1, :3] = [1.0, -0.5, 0.3]
        out["M=1 " + label] = (Problem(6, [FIXED, FIXED], mode_x, np.array([0.0, 3.0]), xn), np.array(X0, dtype=np.float64), 20)
    M, N, tf = 3, 20, 1.8
    X0 = np.array(X0_DINT)
    nodes = [X0] + [np.array(hm.integrate("dint", DINT_P, (0.0, 0.0), 0.0, k * tf / M, X0, N)[-1]) for k in (1, 2)]
    mode_x = np.zeros((M + 1, 6), dtype=np.int32)
    mode_x[1:M] = CONTINUOUS
    mode_x[M, 3:] = FREE
    xn = np.zeros((M + 1, 12))
    xn[0, :6] = X0[:6]
    xn[M, :6] = 0.3
    prob = Problem(6, [FIXED, FREE, CONTINUOUS, FREE], mode_x, np.array([0.0, 0.6, 1.2, 1.8]), xn)
    z = np.concatenate([np.concatenate(nodes), [0.55, 1.9]])
    z[12 + 9:12 + 12] *= 8.0                                            # segment 1 saturates the control
    out["M=3 free interior and final time"] = (prob, z, N)
    return out


_JAC = {}


def jacobians(case, model):
    """(J in doubles, J in 240 bits) of the restated exact Jacobian, computed once."""
    if (case, model) not in _JAC:
        prob, z, N = dint_hx_cases()[case]
        with hx.entries():
            J, _ = ejr.exact_jacobian_row(model, DINT_P, (0.0, 0.0), prob, z, N)
            Jh, _ = ejr.exact_jacobian_row(model, DINT_P, (0.0, 0.0), prob, z, N, high=True)
        _JAC[(case, model)] = (J, Jh)
    return _JAC[(case, model)]


def deviation(J, Jh):
    return max(abs(mpf(float(a)) - q) for a, q in zip(np.asarray(J).ravel(), np.asarray(Jh).ravel()))


@pytest.mark.parametrize("name", cpu.ALL_MODELS)
def test_5_the_matrix_in_doubles_against_240_bits(name):
    model, P, sw, t, X = cpu.points(name, count=6)
    worst = 0.0
    for k in range(len(X)):
        A, _ = hx.hamiltonian_jacobian(model, P, sw, t[k], X[k])
        Ah, _ = hx.hamiltonian_jacobian(model, P, sw, t[k], X[k], high=True)
        worst = max(worst, float(deviation(A, Ah) / amax(Ah)))
    record("5", "%-16s max |A_double - A_240| / max|A| over 6 points = %.3e" % (name, worst))
    assert np.isfinite(worst)


@pytest.mark.parametrize("case", ["M=1 unsaturated", "M=3 free interior and final time"])
def test_5_the_exact_jacobian_of_dint_hx_against_its_240_bit_recurrence(case):
    J, Jh = jacobians(case, "dint_hx")
    dev = deviation(J, Jh)
    record("5", "dint_hx exact Jacobian %-34s max |J_double - J_240| = %.3e  (|J| = %.3e)" % (case, float(dev), float(amax(Jh))))
    assert mpf(0) <= dev < mpf("inf")


# ---- (6) the H-only model and the hand-written one are the same problem ---------------------------------------------------------------

@pytest.mark.parametrize("case", ["M=1 unsaturated", "M=1 saturated"])
def test_6_exact_jacobian_of_dint_hx_and_of_the_in_tree_double_integrator(case):
    Jx, Jxh = jacobians(case, "dint_hx")
    Jd, Jdh = jacobians(case, "dint")
    gap = float(np.max(np.abs(Jx - Jd)))
    allowed = 8 * (deviation(Jx, Jxh) + deviation(Jd, Jdh))
    record("6", "exact Jacobian %-18s |J_hx - J_dint| = %.3e, own deviations %.3e + %.3e, ratio to the allowance %.3f"
           % (case, gap, float(deviation(Jx, Jxh)), float(deviation(Jd, Jdh)), float(gap / allowed) if allowed else 0.0))
    assert gap <= allowed


@pytest.mark.parametrize("X0, label", [(X0_DINT, "unsaturated"), (X0_DINT_SAT, "saturated")])
def test_6_phi_of_dint_hx_and_of_the_in_tree_double_integrator(X0, label):
    N, t2 = 20, 3.0
    phi, dev = {}, {}
    with hx.entries():
        for model in ("dint_hx", "dint"):
            phi[model] = fr.fields_segment(model, DINT_P, (0.0, 0.0), 6, 0.0, t2, X0, N, cols=fr.ALL)["phi"]
            high = fr.fields_segment(model, DINT_P, (0.0, 0.0), 6, 0.0, t2, X0, N, cols=fr.ALL, cls=fr.DualMpf, kit=fr.DualMpfKit())["phi"]
            dev[model] = deviation(phi[model], np.array(high, dtype=object))
    gap = float(np.max(np.abs(phi["dint_hx"] - phi["dint"])))
    allowed = 8 * (dev["dint_hx"] + dev["dint"])
    record("6", "Phi %-12s 20 steps: |Phi_hx - Phi_dint| = %.3e, own deviations %.3e + %.3e, ratio to the allowance %.3f"
           % (label, gap, float(dev["dint_hx"]), float(dev["dint"]), float(gap / allowed) if allowed else 0.0))
    assert gap <= allowed


# ---- (7) the mutations are caught ------------------------------------------------------------------------------------------------------

# mutation -> the points it applies to.  sqrt_inner_of_s needs a root in the text.  drop_inner_cross needs a product one of whose
# factors has a second derivative of its own (a.d[k].d != 0): osc1d's H is quadratic, every factor of its products is linear in X, the
# dropped term is an exact zero there (measured: off by 0.0) and the mutation does not apply to it
MUTATION_POINTS = {
    "outer_shifted": ["dint unsaturated", "dint saturated", "goddard smooth mu2=1 interior", "goddard general full thrust", "covid clamp=None above=True", "osc1d"],
    "drop_inner_cross": ["dint unsaturated", "dint saturated", "goddard smooth mu2=1 interior", "goddard general full thrust", "covid clamp=None above=True"],
    "sqrt_inner_of_s": ["dint unsaturated", "dint saturated", "goddard smooth mu2=1 interior", "goddard general full thrust"],
}


@pytest.mark.parametrize("mutate, name", [(m, n) for m, names in MUTATION_POINTS.items() for n in names])
def test_7_wrong_restatements_miss_the_matrix(mutate, name):
    model, P, sw, t, X, _ = INSIDE[name]
    A, _ = a240(name)
    Am, _ = hx.hamiltonian_jacobian(model, P, sw, t, X, high=True, mutate=mutate)
    miss = amax(A - Am) / amax(A)
    record("7", "%-18s %-34s off by %.3e of the matrix's scale" % (mutate, name, float(miss)))
    assert miss > mpf(10) ** -3


def test_7_a_dropped_parameter_derivative_shows_in_a_parameter_sensitivity():
    """plain_param leaves A and the exact Jacobian alone (the parameters are plain doubles there) and is visible in dF/dtheta only:
    the sensitivity of dint_hx's residual to a_max and u_max on a row with a saturated segment."""
    prob, z, N = dint_hx_cases()["M=3 free interior and final time"]
    dirs = [(sr.DIR_PARAM, 0), (sr.DIR_PARAM, 1), (sr.DIR_PARAM, 2)]
    with hx.entries():
        G = sr.sensitivity_g("dint_hx", DINT_P, (0.0, 0.0), prob, z, N, dirs)
        Gd = sr.sensitivity_g("dint", DINT_P, (0.0, 0.0), prob, z, N, dirs)
        hx.MUTATE_RHS[0] = "plain_param"
        try:
            Gm = sr.sensitivity_g("dint_hx", DINT_P, (0.0, 0.0), prob, z, N, dirs)
        finally:
            hx.MUTATE_RHS[0] = None
    scale = np.max(np.abs(G))
    assert np.max(np.abs(G - Gd)) <= 1e-10 * scale, "the H-only model's sensitivities are the hand-written model's, to rounding"
    for k, label in enumerate(("u_max", "a_max")):
        miss = np.max(np.abs(G[k] - Gm[k])) / np.max(np.abs(G[k]))
        record("7", "plain_param         dF/d%-6s of dint_hx, M = 3, a saturated segment: off by %.3e of its scale" % (label, miss))
        assert miss > 1e-3
    A, _ = hx.hamiltonian_jacobian("dint", DINT_P, (0.0, 0.0), 0.0, X0_DINT_SAT)
    Am, _ = hx.hamiltonian_jacobian("dint", DINT_P, (0.0, 0.0), 0.0, X0_DINT_SAT, mutate="plain_param")
    assert np.array_equal(bits(A), bits(Am)), "with plain parameters the mutation changes nothing"


# ---- (8) texts and symbols -------------------------------------------------------------------------------------------------------------

def test_8_abi_plugins_symbols_and_header():
    launch = open(os.path.join(ROOT, "socp_amd", "csrc", "launch.hpp")).read()
    assert "kPluginAbi = 17" in launch and "kPluginAbi = 16:" in launch
    for name in ("osc1d_hx_plugin.hip", "dint_hx_plugin.hip"):
        text = open(os.path.join(ROOT, "tests", "plugin", name)).read()
        assert "SOCP_DEFINE_HAMILTONIAN_PLUGIN_EXACT" in text and "hamiltonian_t" in text
        assert " rhs(" not in text and "rhs_t" not in text, "no hand-written dynamics"
    import ctypes
    from socp_amd import capi
    lib = ctypes.CDLL(capi.LIB_PATH)
    for sym in ("socp_ctx_has_hamiltonian_jacobian", "socp_hamiltonian_jacobian_batch_dev", "socp_hamiltonian_jacobian_batch"):
        assert hasattr(lib, sym), sym
    header = open(os.path.join(ROOT, "include", "socp_hip.h")).read()
    assert "NESTED DUAL NUMBERS" in header and "socp_hamiltonian_jacobian_batch" in header
    assert "SOCP_DEFINE_HAMILTONIAN_PLUGIN_EXACT" in open(os.path.join(ROOT, "include", "socp_plugin.h")).read()


def test_8_the_lent_entries_are_taken_back():
    with hx.entries():
        assert "dint_hx" in fr.RHS and "dint_hx" in ejr.HAMILTONIAN and ejr.SWITCHING_READS_XP["dint_hx"]
    assert not set(hx.BASE) & (set(fr.RHS) | set(ejr.HAMILTONIAN) | set(ejr.SWITCHING_READS_XP))
