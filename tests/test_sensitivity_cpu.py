"""CPU: the definition of socp_sensitivity_batch as tests/sensitivity_reference.py restates it.
(1) G in doubles against the same recurrence on 240-bit dual numbers, beside the exact Jacobian's own columns on the same case;
(2) the 240-bit G against 240-bit central differences in theta of the 240-bit residual, every direction kind, on Goddard M = 1,
    Goddard M = 3 with a free tf in both laws, the double integrator with a FIXED interior node and a free tf, and covid19;
(3) the instrument: wrong restatements fail (2); (4) the tangent predictor on the nominal Goddard extremal, exact against forward
    differences; (5) the symbols.  No GPU; the library is only asked for its symbols.

Measured (profiles/sensitivity_cpu_tests.txt): see the lines of the run on record there."""
import os

import numpy as np
import pytest

import exact_jacobian_reference as ej
import fields_reference as fr
import sensitivity_cases as sc
import sensitivity_reference as sr
import tangent_reference as tr

pytestmark = pytest.mark.skipif(not fr.HAVE_MPMATH, reason="mpmath is the 240-bit carrier")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mpf = fr.mpf


def record(key, line):
    """The figures of a run (pytest -s): profiles/sensitivity_cpu_tests.txt keeps the lines of the run on record."""
    print("[sensitivity_cpu %s] %s" % (key, line))


def column_deviation(A, truth):
    """The largest over the rows of A (directions, or columns of a matrix given transposed) of max|a - truth| / max|truth|; a row
    whose truth is all zero must be all zero."""
    worst = mpf(0)
    for a, q in zip(A, truth):
        big = max(abs(v) for v in q)
        if big == 0:
            assert not np.any(np.asarray(a, dtype=np.float64)), "an identically zero row is exactly zero"
            continue
        worst = max(worst, max(abs(mpf(float(x)) - v) for x, v in zip(a, q)) / big)
    return worst


# ---- (1) the doubles beside the 240-bit recurrence -------------------------------------------------------------------------------

def test_1_g_in_doubles_against_240_bits():
    """Nominal Goddard, M = 1, N = 50, the eight parameters and both node times.  The bar: 8 x the largest deviation of the exact
    Jacobian's own columns from their 240-bit values on this case -- G runs the same operations plus the parameter's dual products.
    The deviation of a direction or a column is max|a - truth| / max|truth| over its rows.  The exact Jacobian's columns are the 14
    state columns and its LENGTH column: with t_f fixed the matrix has none, so that one is taken from the same row with t_f FREE
    (rows 0 .. 13: the Hamiltonian row is not part of G).  A TIME direction IS that column times w = +-1, bit for bit."""
    from oracle.oracle import Problem, FIXED, FREE
    c = sc.goddard_single()
    z, N, prob = c["Z"][0], 50, c["prob"]
    dirs = [d for d in c["dirs"] if d[0] != tr.DIR_XNODE]
    args = ("goddard", c["params"], c["sw"], prob, z, N)
    G, Gh = sr.sensitivity_g(*args, dirs), sr.sensitivity_g(*args, dirs, high=True)
    J, _ = ej.exact_jacobian_row(*args)
    Jh, _ = ej.exact_jacobian_row(*args, high=True)
    free = ("goddard", c["params"], c["sw"], Problem(7, [FIXED, FREE], prob.mode_x, prob.time, prob.xnode), np.append(z, prob.time[1]), N)
    L, Lh = ej.exact_jacobian_row(*free)[0][:14, 14], ej.exact_jacobian_row(*free, high=True)[0][:14, 14]
    assert np.array_equal(G[9].view(np.uint64), L.view(np.uint64)) and np.array_equal(G[8], -L), "the TIME directions are the length column"
    dev_p = column_deviation([G[k] for k, d in enumerate(dirs) if d[0] == tr.DIR_PARAM], [Gh[k] for k, d in enumerate(dirs) if d[0] == tr.DIR_PARAM])
    dev_g, dev_s, dev_l = column_deviation(G, Gh), column_deviation(J.T, Jh.T), column_deviation([L], [Lh])
    dev_j = max(dev_s, dev_l)
    record("1", "nominal Goddard M = 1, N = 50, largest deviation from 240 bits: G %.3e (its parameter directions %.3e); the exact Jacobian's "
           "columns %.3e (state columns %.3e, length column %.3e); ratio %.3f (bar 8), parameter directions to state columns %.3f"
           % (float(dev_g), float(dev_p), float(dev_j), float(dev_s), float(dev_l), float(dev_g / dev_j), float(dev_p / dev_s)))
    assert dev_g <= 8 * dev_j and dev_p <= 8 * dev_s


# ---- (2) the 240-bit G against central differences of the 240-bit residual ------------------------------------------------------------

_DEV = {}


def central_deviation(name, mutate=()):
    """max over the case's directions and rows of |G - (F(theta + h) - F(theta - h)) / 2h| / max|G|, h = 1e-20 max(1, |theta|), all
    in 240 bits; the differences are computed once per case."""
    c = sc.CASES[name]()
    z = c["Z"][0]
    args = (c["model"], c["params"], c["sw"], c["prob"], z, c["N"])
    G = sr.sensitivity_g(*args, c["dirs"], high=True, mutate=mutate)
    if name not in _DEV:
        cds = []
        for kind, index in c["dirs"]:
            h = mpf(10) ** -20 * max(1.0, abs(sr.theta_of(c["params"], c["prob"], kind, index)))
            Fp, Fm = (sr.residual_high(*args, move=(kind, index, s * h)) for s in (1, -1))
            cds.append([(a - b) / (2 * h) for a, b in zip(Fp, Fm)])
        _DEV[name] = cds
    cds = _DEV[name]
    big = max(abs(v) for row in cds for v in row)
    worst = max(abs(g - q) for row, cd in zip(G, cds) for g, q in zip(row, cd))
    return worst / big, G, c


# Truncation is h^2 = 1e-40 of the third derivative's scale and rounding 1e-72 / h = 1e-52, so 1e-30 of max|G| is safe and still sees
# any dropped term: a wrong restatement is off by more than 1e-3 (check 3).
TOL_2 = 1e-30


@pytest.mark.parametrize("name", ["goddard_single", "goddard_m3", "goddard_m3_general", "dint_fixed_node_free_tf", "covid_m2", "osc1d_plugin"])
def test_2_g_against_central_differences(name):
    dev, G, c = central_deviation(name)
    record("2 " + name, "240-bit G against 240-bit central differences in theta (h = 1e-20 max(1, |theta|)), %d directions: %.3e of max|G| "
           "(bar %.0e)" % (len(c["dirs"]), float(dev), TOL_2))
    kinds = {k for k, _ in c["dirs"]}
    assert kinds == {tr.DIR_PARAM, tr.DIR_TIME, tr.DIR_XNODE}, "every direction kind"
    for k in c["unread"]:
        assert all(v == 0 for v in G[k]), "an entry that is never read gives G = 0"
    read = [k for k in range(len(c["dirs"])) if k not in c["unread"]]
    assert sum(1 for k in read if any(v != 0 for v in G[k])) >= len(read) - 2, "the directions that are read move the residual"
    assert dev <= TOL_2


# ---- (3) the instrument ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mutation", sr.MUTATIONS)
def test_3_wrong_restatements_fail_check_2(mutation):
    devs = {name: float(central_deviation(name, mutate=(mutation,))[0]) for name in ("goddard_m3", "dint_fixed_node_free_tf", "covid_m2")}
    record("3 " + mutation, "wrong restatement %-22s deviation in check 2: %s" % (mutation, ", ".join("%s %.3e" % kv for kv in devs.items())))
    assert max(devs.values()) > 1e-3, "a wrong restatement is off by far more than the bar of check 2"


# ---- (4) the tangent predictor on the nominal Goddard extremal -----------------------------------------------------------------------

RELS = (0.02, 0.01, 0.005)
_PRED = {}


def predictor_case(mu2, index):
    """(errors of z + dtheta dz against the re-polished root at theta (1 + rel), rel in RELS) for the exact dz and for the forward-
    difference tangent's, at the polished root of newton_cases.goddard(mu2), N = 50."""
    if (mu2, index) not in _PRED:
        import newton_cases as nc
        import newton_reference as nr
        c = nc.goddard(mu2)
        o, prob, root, N = c["o"], c["prob"], c["root"], c["N"]
        P = np.array(c["params"], dtype=np.float64)
        dirs = [(tr.DIR_PARAM, index)]
        dz_exact = sr.sensitivity_row("goddard", P, (0.0, 0.0), prob, root, N, dirs)["dz"][0]
        dz_fd = tr.tangent_reference(o, prob, 8, root[None], dirs, epsfcn=1e-15, jac=0)["dz"][0][0]

        def solve_at(theta, start):
            block = np.concatenate([P, [0.0, 0.0]])
            block[index] = theta
            r = nr.newton_reference("goddard", o, prob, 8, N, start[None], nc.POLISH, params=block[None])
            assert r["rnorm"][0] <= 1e-9, "the polish converged"
            return r["z"][0]

        roots = {rel: solve_at(P[index] * (1.0 + rel), root + P[index] * rel * dz_exact) for rel in RELS}
        err = lambda dz: [float(np.linalg.norm(root + P[index] * rel * dz - roots[rel])) for rel in RELS]      # noqa: E731
        _PRED[(mu2, index)] = (err(dz_exact), err(dz_fd))
    return _PRED[(mu2, index)]


@pytest.mark.parametrize("mu2,index,what", [(1.0, 2, "KD"), (1.0, 0, "C"), (0.2, 2, "KD")])
def test_4_the_exact_predictor_is_second_order(mu2, index, what):
    exact, fd = predictor_case(mu2, index)
    ratios = [exact[i] / exact[i + 1] for i in range(2)]
    record("4 mu2=%g %s" % (mu2, what), "predictor error at rel = 2 %% / 1 %% / 0.5 %%: exact %s, forward difference %s; exact ratios per halving %s, "
           "forward-difference %s" % (" / ".join("%.3e" % v for v in exact), " / ".join("%.3e" % v for v in fd),
                                      ", ".join("%.3f" % r for r in ratios), ", ".join("%.3f" % (fd[i] / fd[i + 1]) for i in range(2))))
    assert all(3.5 <= r <= 4.5 for r in ratios), ratios
    if (mu2, what) == (0.2, "KD"):
        assert exact[2] < fd[2] / 3.0, (exact[2], fd[2])


# ---- (5) the surface ---------------------------------------------------------------------------------------------------------------

def test_5_abi_header_and_symbols():
    """Fails without the feature."""
    assert "kPluginAbi = 15" in open(os.path.join(ROOT, "socp_amd", "csrc", "launch.hpp")).read()
    header = open(os.path.join(ROOT, "include", "socp_hip.h")).read()
    names = ("socp_ctx_has_sensitivity", "socp_sensitivity_batch_dev", "socp_sensitivity_batch", "socp_sensitivity_batch_blocks")
    for name in names:
        assert "int %s(" % name in header, name
    assert "size_t socp_sensitivity_work_bytes(" in header
    from socp_amd import capi
    L = capi.lib()
    for name in names + ("socp_sensitivity_work_bytes",):
        assert hasattr(L, name), name
    for name in ("has_sensitivity", "sensitivity_work_bytes", "sensitivity_batch_dev", "sensitivity_batch"):
        assert callable(getattr(capi.Context, name)), name
