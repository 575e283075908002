"""CPU: the definition of socp_exact_jacobian_batch as tests/exact_jacobian_reference.py restates it.
(1) the restated hamiltonian_t / switching_fn_t against the oracle's Hamiltonian, bit for bit, and the restated residual against
    the oracle's; (2) nominal Goddard, M = 1, N = 50: the restatement in doubles and the oracle's forward difference against the same
    recurrence on 240-bit dual numbers; (3) the free-time column and the Hamiltonian / switching rows of the 240-bit dual evaluation
    against 240-bit central differences of the 240-bit residual; (4) the instrument: wrong restatements fail (3); (5) the symbols.
No GPU; the library is only asked for its symbols.

Measured (profiles/exact_jacobian_cpu_tests.txt), max|J - truth| / max|truth| on nominal Goddard, exact / forward difference:
mu2 = 1: 1.5e-13 / 7.8e-2 (ratio 2.0e-12), mu2 = 0.2: 2.6e-13 / 7.7e-3 (ratio 3.4e-11); the bar is 1e-3.  (The whole matrix: the
columns of the initial velocity, |v| = 1.7e-10, are where the difference fails; the 1.5e-4 on record is for the block dx/dp alone.)
(3): the dual evaluation and the central differences (step 2^-80) differ by 1.2e-45 (Goddard) and 8.6e-49 (double integrator) of the
scale, the columns of the FREE nodes 2 and 4 of the n = 87 structure (the `1.0 - q` weight) by 3.5e-48; the bar is 1e-40.  (4): the wrong
restatements are off by 1.4e-2 ... 0.68; "drop_hd_length" coincides with "no_length" (see test_4)."""
import os

import numpy as np
import pytest

import exact_jacobian_reference as ej
import fields_reference as fr
import jacobi_cases as jc
from conftest import goddard_single_problem

pytestmark = pytest.mark.skipif(not fr.HAVE_MPMATH, reason="mpmath is the 240-bit carrier")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GODDARD_SETTINGS = {"mu2=1": (1.0, (0.0, 0.0)), "mu2=0.2": (0.2, (0.0, 0.0)), "mu2=0": (0.0, (0.05, 0.15))}


def record(key, line):
    """The figures of a run (pytest -s): profiles/exact_jacobian_cpu_tests.txt keeps the lines of the run on record."""
    print("[exact_jacobian_cpu %s] %s" % (key, line))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def goddard_oracle(mu2, sw, n):
    from oracle.oracle import Oracle, MODEL_GODDARD
    o = Oracle(MODEL_GODDARD, step_nbr=n)
    o.set_param("mu2", mu2)
    o.set_switching(list(sw))
    return o


# ---- (1) the restatement is tied to the reference ----------------------------------------------------------------------------------

@pytest.mark.parametrize("setting", list(GODDARD_SETTINGS))
def test_1_goddard_hamiltonian_equals_the_oracle(setting):
    from test_fields_cpu import goddard_rows
    mu2, sw = GODDARD_SETTINGS[setting]
    o = goddard_oracle(mu2, sw, 50)
    P = o.params()[:8]
    X, t = goddard_rows(np.random.default_rng(21), 400, sw)
    for k in range(400):
        H = o.hamiltonian(t[k], X[k])
        assert bits(H) == bits(ej.plain_hamiltonian("goddard", P, sw, t[k], X[k])), k
        assert bits(H) == bits(ej.plain_switching("goddard", P, sw, t[k], X[k], X[(k + 1) % 400])), "Goddard's row is H(t, X-)"
    assert not ej.SWITCHING_READS_XP["goddard"]


@pytest.mark.parametrize("model", ["dint", "covid"])
def test_1_dint_and_covid_hamiltonian_equal_the_oracle(model):
    from test_fields_cpu import dint_oracle, covid_oracle
    rng = np.random.default_rng(22)
    if model == "dint":
        o = dint_oracle()
        P = o.params()[:3]
        rows = [rng.uniform(-1.0, 1.0, 12) * rng.choice([0.3, 3.0]) for _ in range(400)]
    else:
        o = covid_oracle()
        P = o.params()[:8]
        rows = [np.concatenate([rng.uniform(0.0, 1.0, 4) * [1.0, 0.05, 0.3, 0.3], rng.uniform(-1.0, 1.0, 4) * rng.choice([0.01, 1e3])]) for _ in range(400)]
    seen = set()
    for k, X in enumerate(rows):
        K = fr.PlainKit()
        H = ej.hamiltonian_on(model, K, [float(p) for p in P], [0.0, 0.0], 0.0, [float(x) for x in X])
        seen |= {n for n, m in K.margins.items() if (m <= 0 if n == "u-umin" else m >= 0)}
        assert bits(o.hamiltonian(0.0, X)) == bits(H), k
        Xp = rows[(k + 1) % 400]
        assert bits(o.hamiltonian(0.0, X) - o.hamiltonian(0.0, Xp)) == bits(ej.plain_switching(model, P, (0.0, 0.0), 0.0, X, Xp)), k
    assert seen == ({"|u|-umax"} if model == "dint" else {"u-umin", "u-umax", "I-Imax"}), "every branch was taken somewhere"
    assert ej.SWITCHING_READS_XP[model]


def m3_case(N=6):
    c = dict(jc.goddard_m3(B=2, seed=9), N=N)
    c["o"] = jc.goddard_oracle(N)
    return c


def dint_free_interior_case(N=6):
    """M = 2 with a FREE interior time (the unknown 24) and a CONTINUOUS interior state; segment 1 saturates the control."""
    from oracle.oracle import Oracle, Problem, MODEL_DINT, FIXED, FREE, CONTINUOUS
    o = Oracle(MODEL_DINT, step_nbr=N)
    n0 = np.array([0.0, 0.0, 0.0, 0.3, -0.2, 0.1, 0.02, -0.01, 0.015, 0.4, -0.3, 0.2])
    n1 = np.array([0.5, -0.3, 0.2, 0.1, 0.1, -0.2, 0.02, -0.01, 0.015, 2.0, -1.5, 1.0])
    mode_x = np.zeros((3, 6), dtype=np.int32)
    mode_x[1] = CONTINUOUS
    mode_x[2, 3:] = FREE
    X = np.zeros((3, 12))
    X[2, :3] = [1.0, -0.5, 0.3]
    prob = Problem(6, [FIXED, FREE, FIXED], mode_x, np.array([0.0, 1.5, 3.0]), X)
    return dict(model="dint", o=o, prob=prob, N=N, Z=np.concatenate([n0, n1, [1.4]])[None, :], params=o.params()[:3])


def test_1_the_value_parts_are_the_oracle_residual():
    """F of the restatement against the oracle's shooting function, bit for bit: M = 3 Goddard with a free tf, and the double
    integrator with a free interior time (its row is H(X-) - H(X+))."""
    for c in (m3_case(), dint_free_interior_case()):
        for z in c["Z"]:
            _, F = ej.exact_jacobian_row(c["model"], c["params"], (0.0, 0.0), c["prob"], z, c["N"])
            assert np.array_equal(bits(F), bits(c["o"].residual(c["prob"], z))), c["model"]


# ---- (2) accuracy on the nominal Goddard extremal, beside the forward difference -------------------------------------------------

@pytest.mark.parametrize("setting", ["mu2=1", "mu2=0.2"])
def test_2_exact_against_the_forward_difference_on_nominal_goddard(setting):
    mu2, sw = GODDARD_SETTINGS[setting]
    N = 50
    o = goddard_oracle(mu2, sw, N)
    P = o.params()[:8]
    prob, z = goddard_single_problem()
    J, F = ej.exact_jacobian_row("goddard", P, sw, prob, z, N)
    truth, _ = ej.exact_jacobian_row("goddard", P, sw, prob, z, N, high=True)
    Fo = o.residual(prob, z)
    assert np.array_equal(bits(F), bits(Fo))
    Jfd = o.fdjac(prob, z, Fo, epsfcn=0.0)
    big = max(abs(q) for q in truth.ravel())
    dev = lambda A: max(abs(fr.mpf(float(a)) - q) for a, q in zip(np.asarray(A).ravel(), truth.ravel())) / big      # noqa: E731
    d_exact, d_fd = dev(J), dev(Jfd)
    record("2 " + setting, "nominal Goddard %-8s M = 1, N = 50: max|J - truth| / max|truth|: exact %.3e, forward difference %.3e, ratio %.3e"
           % (setting, float(d_exact), float(d_fd), float(d_exact / d_fd)))
    assert d_exact <= fr.mpf(10) ** -3 * d_fd


# ---- (3) the free-time column and the Hamiltonian rows against 240-bit central differences ------------------------------------------

H80 = None if not fr.HAVE_MPMATH else fr.mpf(2) ** -80
_CD = {}


def central_difference(name, c, z, k):
    """Column k of dF/dz by (F(z + h e_k) - F(z - h e_k)) / 2h on the 240-bit residual, h = 2^-80; computed once."""
    if (name, k) not in _CD:
        sides = []
        for sgn in (1, -1):
            zz = [fr.mpf(float(v)) for v in z]
            zz[k] = zz[k] + sgn * H80
            sides.append(ej.exact_jacobian_row(c["model"], c["params"], (0.0, 0.0), c["prob"], zz, c["N"], high=True, derivs=False)[1])
        _CD[(name, k)] = [(a - b) / (2 * H80) for a, b in zip(*sides)]
    return _CD[(name, k)]


# The allowed difference is the central difference's own truncation, h^2 / 6 |F'''| with h^2 = 2^-160 = 6.8e-49, beside its rounding
# 2^-240 / h = 7e-49 of |F|: 1e-40 of the scale allows third derivatives up to 1e8 of it (the segments differentiated here start from
# states of order one; the start with |v| = 1.7e-10 enters only through the step length).  A wrong restatement is off by order one.
TOL_3 = 1e-40


def goddard_deviation(mutate=()):
    """Goddard, M = 3, FREE tf (n = 43, the interior times interpolated: weights 1/3 and 2/3): the free-time column 42 (all rows) and
    the Hamiltonian row 42 (the columns of the last segment, and two of segment 0, which it does not depend on)."""
    c = m3_case(N=4)
    z = c["Z"][0]
    n = c["prob"].n
    assert n == 43 and ej.Layout(c["prob"]).ft_row[3] == 42
    J, _ = ej.exact_jacobian_row("goddard", c["params"], (0.0, 0.0), c["prob"], z, c["N"], high=True, mutate=mutate)
    scale = max(1, max(abs(q) for q in J.ravel()))
    worst = max(abs(J[r, 42] - q) for r, q in enumerate(central_difference("goddard_m3", c, z, 42)))
    for k in [3, 10] + list(range(28, 42)):
        worst = max(worst, abs(J[42, k] - central_difference("goddard_m3", c, z, k)[42]))
    return worst / scale, J


def dint_deviation(mutate=()):
    """The double integrator with a FREE interior time: EVERY column -- the free-time column 24, the switching row 24 with its
    -grad H(X+) part, the continuity block and the -I beside it."""
    c = dint_free_interior_case()
    z = c["Z"][0]
    n = c["prob"].n
    assert n == 25 and ej.Layout(c["prob"]).ft_row[1] == 24
    J, _ = ej.exact_jacobian_row("dint", c["params"], (0.0, 0.0), c["prob"], z, c["N"], high=True, mutate=mutate)
    scale = max(1, max(abs(q) for q in J.ravel()))
    worst = max(abs(J[r, k] - q) for k in range(n) for r, q in enumerate(central_difference("dint_free", c, z, k)))
    return worst / scale, J


def n87_deviation():
    """The free-switching-time structure (M = 6, n = 87: FREE nodes 2, 4 and 6, the odd nodes interpolated) with the smooth law, so
    that the residual depends on the free times through the lengths alone: the columns 84 and 85 of the FREE nodes 2 and 4 (all
    rows).  A FREE junction a FOLLOWED by an interpolated node takes the `1.0 - q` branch of c(j, f): w = (1 - 1/2) - 1 there, which
    neither case above reaches."""
    from oracle.oracle import Problem, FREE
    from test_move_batch_cpu import stage4_structure, stage4_times, GOLD
    z = np.array(GOLD["goddard_N10_M6"][3]["z"])
    mode_xf = np.zeros(7, dtype=np.int32)
    mode_xf[3:7] = FREE
    mode_t, mode_x = stage4_structure(mode_xf)
    X = np.zeros((7, 14))
    X[0, :7] = [0.999949994, 1e-4, 0.01, 1e-10, 1e-10, 1e-10, 1.0]
    X[6, 0] = 1.01
    prob = Problem(7, mode_t, mode_x, stage4_times(z[-1]), X)
    lay = ej.Layout(prob)
    assert prob.n == 87 and lay.kind[2] == 84 and lay.kind[4] == 85 and lay.kind[3] == -2 and (lay.lo[3], lay.hi[3]) == (2, 4)
    c = dict(model="goddard", params=[3.5, 7.0, 310.0, 500.0, 1.0, 1.0, 1.0, -1.0], prob=prob, N=3)
    J, _ = ej.exact_jacobian_row("goddard", c["params"], (0.0, 0.0), prob, z, c["N"], high=True)
    scale = max(1, max(abs(q) for q in J.ravel()))
    worst = max(abs(J[r, k] - q) for k in (84, 85) for r, q in enumerate(central_difference("goddard_n87", c, z, k)))
    return worst / scale, J


def test_3_free_time_column_and_hamiltonian_rows_against_central_differences():
    g, Jg = goddard_deviation()
    d, Jd = dint_deviation()
    record("3", "240-bit dual evaluation against 240-bit central differences (step 2^-80), of the scale: Goddard M = 3 free tf %.3e, "
           "double integrator free interior time %.3e (bar %.0e)" % (float(g), float(d), TOL_3))
    for rows in (range(14, 28), range(28, 42), range(7, 14), (42,)):
        # (the Hamiltonian is nearly conserved along the flow: its own entry is small, not zero)
        assert max(abs(Jg[r, 42]) for r in rows) > 1e-7, "the free-time column reaches the rows of every segment"
    assert any(abs(Jd[24, k]) > 1e-3 for k in range(12, 24)), "the -grad H(X+) part of the switching row"
    assert g <= TOL_3 and d <= TOL_3


def test_3_the_one_minus_q_weight_against_central_differences():
    e, J = n87_deviation()
    record("3 n87", "240-bit dual evaluation against 240-bit central differences, columns of the FREE nodes 2 and 4 of the n = 87 structure: "
           "%.3e of the scale (bar %.0e)" % (float(e), TOL_3))
    # node 2's time moves the rows of segments 0 .. 3, node 4's those of segments 2 .. 5: both signs of w occur
    for k, rows in ((84, (range(14, 28), range(28, 42), range(42, 56), range(56, 70))), (85, (range(42, 56), range(56, 70), range(70, 84), range(7, 14)))):
        for rr in rows:
            assert max(abs(J[r, k]) for r in rr) > 1e-7, (k, rr)
    assert e <= TOL_3


# ---- (4) the instrument ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mutation", ej.MUTATIONS)
def test_4_wrong_restatements_fail_check_3(mutation):
    """Three independent mutations, not four: in the length lane the ONLY source of a derivative is the term h.d F.v, so
    "drop_hd_length" leaves the whole length column zero and coincides with "no_length" (the same deviations, 1.432e-02 and 6.801e-01);
    the issue names it, so it stays.  "no_ci" differs from "no_length" in the entries, not in the largest deviation."""
    g = goddard_deviation(mutate=(mutation,))[0] if mutation != "no_minus_identity" else 0.0
    d = dint_deviation(mutate=(mutation,))[0]
    record("4 " + mutation, "wrong restatement %-18s deviation in check 3: Goddard %.3e, double integrator %.3e" % (mutation, float(g), float(d)))
    assert max(g, d) > 1e-6, "a wrong restatement is off by far more than the bar of check 3"
    assert not (g <= TOL_3 and d <= TOL_3)


# ---- (5) the surface ---------------------------------------------------------------------------------------------------------------

def test_5_abi_header_and_symbols():
    """Fails without the feature."""
    assert "kPluginAbi = 13" in open(os.path.join(ROOT, "socp_amd", "csrc", "launch.hpp")).read()
    header = open(os.path.join(ROOT, "include", "socp_hip.h")).read()
    names = ("socp_ctx_has_exact_jacobian", "socp_exact_jacobian_batch_dev", "socp_exact_jacobian_batch", "socp_exact_jacobian_batch_blocks")
    for name in names:
        assert "int %s(" % name in header, name
    from socp_amd import capi
    L = capi.lib()
    for name in names:
        assert hasattr(L, name), name
    for name in ("has_exact_jacobian", "exact_jacobian_batch_dev", "exact_jacobian_batch"):
        assert callable(getattr(capi.Context, name)), name
