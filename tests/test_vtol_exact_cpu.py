"""CPU: vtolUAV in the exact-derivative stack as tests/vtol_exact_reference.py restates it -- the tanh rule, the model's texts over
a number type, custom final rows (final_row_t) and the switching_state rows of a FREE state component of an interior node
(switching_state_t with kSwitchingStateXpContinuous).  Stages path_1 (n = 13, M = 1: all-FREE custom final rows) and path_2
(n = 26: the interior node's positions FREE -- hook rows --, its velocities CONTINUOUS, both times FREE) of
tests/golden/vtol_flow.npz at their stored solutions, ca = alphaV = 0.05, the shipped map, N = 10 steps per segment.
(1) the value parts of the texts equal vtol_reference.vtol_ref on F64Kit bit for bit, and the states are away from the kinks;
(2) the whole 240-bit matrix against central differences (step 2^-80) of the 240-bit residual, within 1e-40 of max|J| -- the bar
of tests/test_hamiltonian_exact_cpu.py for the same construction; (3) six wrong restatements are each off by a stated share of the
scale; (4) the double-precision restatement against the 240-bit matrix (dev_ref), shipped and EMPTY map, and the fixture
tests/golden/vtol_exact_pin.npz holds these matrices; (5) Newton in numpy on the restated Jacobian (tests/newton_reference.py's
iteration) converges from all 8 starts of every stage with the factor 1e-5; (6) texts and symbols.  No GPU.
The figures are written to profiles/vtol_exact_cpu_tests.txt."""
import os

import numpy as np
import pytest

import fields_reference as fr
import vtol_exact_reference as vx
from fields_reference import mpf

pytestmark = pytest.mark.skipif(not fr.HAVE_MPMATH, reason="mpmath is the 240-bit carrier")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
PROFILE = os.path.join(ROOT, "profiles", "vtol_exact_cpu_tests.txt")
H80 = mpf(2) ** -80 if fr.HAVE_MPMATH else None  # the step of the 240-bit central differences
TOL_FD = 1e-40                                  # their bar: truncation h^2 / 6 |F'''| with h^2 = 6.8e-49, rounding 2^-240 / h = 7e-49
NEWTON_FACTOR = 1e-5
# the decision margins a state must keep: |norm_u - u_max| (the saturation boundary), the distance to a box's centre plane, the speed
MARGIN_FLOOR = {"norm_u-u_max": 1e-3, "box centre plane": 1e-3, "normV": 1e-6}
FLOW = np.load(os.path.join(GOLD, "vtol_flow.npz"))
SHIPPED = np.load(os.path.join(GOLD, "vtol_vectors.npz"))["table_shipped"]
EMPTY = np.zeros((0, 7))
_FIG, _HIGH, _DOUBLE = {}, {}, {}


def record(key, line):
    """One figure line; the profile file is rewritten whole, in key order, every time (a read-only tree keeps the print)."""
    print("[vtol_exact_cpu %s] %s" % (key, line))
    _FIG[key] = line
    try:
        with open(PROFILE, "w") as f:
            f.write("tests/test_vtol_exact_cpu.py: vtolUAV stages of tests/golden/vtol_flow.npz at their stored solutions, ca = alphaV = 0.05,\n"
                    "N = 10 RK4 steps per segment, 240-bit mpmath against numpy.float64 (pytest -s prints the same lines)\n\n")
            for k in sorted(_FIG):
                f.write("[%s] %s\n" % (k, _FIG[k]))
    except OSError:
        pass


def bits(a):
    """The integer view of doubles, every NaN the same word: 0 / 0 computed has the sign and payload of the platform, numpy.nan its own."""
    a = np.array(a, dtype=np.float64)
    return np.where(np.isnan(a), np.uint64(0x7FF8000000000000), a.view(np.uint64))


def setting(name):
    return vx.stage(FLOW, name, ca=vx.CA, alphaV=vx.ALPHAV)


def high(name, table_tag):
    """The 240-bit matrix and residual of a stage, computed once."""
    if (name, table_tag) not in _HIGH:
        fr.mpmath.mp.prec = 240
        P, prob, z = setting(name)
        _HIGH[name, table_tag] = vx.exact_jacobian_row(P, SHIPPED if table_tag == "shipped" else EMPTY, prob, z, vx.N_STEPS, high=True)
    return _HIGH[name, table_tag]


def double(name, table_tag):
    if (name, table_tag) not in _DOUBLE:
        P, prob, z = setting(name)
        margins, ends = {}, []
        J, F = vx.exact_jacobian_row(P, SHIPPED if table_tag == "shipped" else EMPTY, prob, z, vx.N_STEPS, margins=margins, end_states=ends)
        _DOUBLE[name, table_tag] = (J, F, margins, ends)
    return _DOUBLE[name, table_tag]


# ---- 1. the tie to the reference's restatement, and the margins ----------------------------------------------------------------------

@pytest.mark.parametrize("name", vx.STAGES)
def test_value_parts_are_vtol_ref_bit_for_bit(name):
    P, prob, z = setting(name)
    _, _, margins, ends = double(name, "shipped")
    states = [z[vx.S * i:vx.S * (i + 1)] for i in range(prob.M)] + [np.array(e, dtype=np.float64) for e in ends]
    # and the corners: a state at rest (rows 9-11 NaN), one on a box's centre plane (the reset), a saturated control
    rest = states[0].copy()
    rest[3:6] = 0.0
    plane = states[0].copy()
    plane[0] = SHIPPED[0, 1]
    sat = states[0].copy()
    sat[9:12] = [-40.0, 30.0, 20.0]
    for table in (SHIPPED, EMPTY):
        for X in states + [rest, plane, sat]:
            (d, H), (dr, Hr) = vx.plain_texts(P, table, X), vx.reference_texts(P, table, X)
            assert np.array_equal(bits(d), bits(dr)), (name, X, d, dr)
            assert np.array_equal(bits([H]), bits([Hr])), (name, X, H, Hr)
    d_rest = vx.plain_texts(P, SHIPPED, rest)[0]
    assert np.isnan(d_rest[9:12]).all() and np.isfinite(d_rest[:9]).all(), "rows 9-11 NaN at rest and nowhere else"
    assert vx.plain_texts(P, SHIPPED, plane)[0][6] == 0.0, "the reset zeroes the whole component"
    for k, floor in MARGIN_FLOOR.items():
        assert float(margins[k]) > floor, (name, k, margins[k])
    record("1 %s" % name, "value parts equal vtol_ref on F64Kit bit for bit at %d states (both maps, and at rest / on a centre plane / saturated); "
           "smallest margins along the trajectory: |norm_u - u_max| %.4g, box centre plane %.4g, normV %.4g"
           % (len(states), margins["norm_u-u_max"], margins["box centre plane"], margins["normV"]))


# ---- 2. the 240-bit matrix against 240-bit central differences ----------------------------------------------------------------------

@pytest.mark.parametrize("name", vx.STAGES)
def test_matrix_against_central_differences_in_240_bits(name):
    P, prob, z = setting(name)
    Jh, Fh = high(name, "shipped")
    n = len(z)
    zz = [mpf(float(v)) for v in z]
    worst = mpf(0)
    for j in range(n):
        zp, zm = list(zz), list(zz)
        zp[j], zm[j] = zz[j] + H80, zz[j] - H80
        Fp = vx.exact_jacobian_row(P, SHIPPED, prob, zp, vx.N_STEPS, high=True, derivs=False)[1]
        Fm = vx.exact_jacobian_row(P, SHIPPED, prob, zm, vx.N_STEPS, high=True, derivs=False)[1]
        worst = max(worst, max(abs((a - b) / (2 * H80) - Jh[i, j]) for i, (a, b) in enumerate(zip(Fp, Fm))))
    scale = vx.amax(Jh)
    record("2 %s" % name, "n = %d: max |J240 - central differences (h = 2^-80) of the 240-bit residual| = %.3e of max|J| = %.6g (bar %.0e)"
           % (n, float(worst / scale), float(scale), TOL_FD))
    assert worst <= TOL_FD * scale
    assert all(Fh[i] == vx.exact_jacobian_row(P, SHIPPED, prob, zz, vx.N_STEPS, high=True, derivs=False)[1][i] for i in range(n)), \
        "the value parts are the residual"


# ---- 3. the wrong restatements -------------------------------------------------------------------------------------------------------

# mutation -> (stage, the least share of max|J| it must be off by).  The shares are orders of magnitude below what the dropped term
# contributes (tanh: an O(phi / mu) gradient through ten steps; the hook: invSigmaXwp = 1 / 60; final_row: invSigmaXwp (nWP_tot - nWP)
# = 0.53 and 0.02; the -1 entries: 1; the length column: |dX/dt|) and 1e8 above the 1e-40 the right restatement keeps
WRONG = {"tanh_no_factor": ("path_2", 1e-6), "hook_no_inv_sigma": ("path_2", 1e-5), "final_no_wp_weight": ("path_1", 1e-4),
         "final_no_002": ("path_1", 1e-5), "hook_no_minus_one": ("path_2", 1e-3), "no_length": ("path_1", 1e-4)}


@pytest.mark.parametrize("mutation", list(WRONG))
def test_wrong_restatements_miss(mutation):
    name, share = WRONG[mutation]
    P, prob, z = setting(name)
    Jh, _ = high(name, "shipped")
    Jm, _ = vx.exact_jacobian_row(P, SHIPPED, prob, z, vx.N_STEPS, mutate=(mutation,))
    J, _, _, _ = double(name, "shipped")
    off, right = vx.dev_of(Jm, Jh), vx.dev_of(J, Jh)
    record("3 %s" % mutation, "%s: off by %.3e of max|J| (must exceed %.0e; the right restatement in doubles: %.3e)" % (name, off, share, right))
    assert off > share and right < 1e-12


# ---- 4. doubles against their 240-bit truth, and the fixture -------------------------------------------------------------------------

@pytest.mark.parametrize("name", vx.STAGES)
@pytest.mark.parametrize("table_tag", ["shipped", "empty"])
def test_doubles_against_240_bits_and_the_fixture(name, table_tag):
    P, prob, z = setting(name)
    Jh, Fh = high(name, table_tag)
    J, F, _, _ = double(name, table_tag)
    dev = vx.dev_of(J, Jh)
    pin = np.load(os.path.join(GOLD, "vtol_exact_pin.npz"))
    key = "%s_%s_" % (name, table_tag)
    record("4 %s %s map" % (name, table_tag), "dev_ref = max |J - J240| / max|J240| = %.3e (fixture %.3e), max|J| = %.6g, |F - F240| = %.3e"
           % (dev, float(pin[key + "dev_ref"]), float(vx.amax(Jh)), float(max(abs(mpf(float(a)) - b) for a, b in zip(F, Fh)))))
    assert dev < 1e-13, "doubles through ten RK4 steps: a few hundred roundings of 1.1e-16"
    assert np.array_equal(pin[key + "J240"], vx.to_double(Jh)) and np.array_equal(pin[key + "F240"], vx.to_double(Fh)), "a stale fixture"
    assert np.array_equal(pin[name + "_z"], z) and np.array_equal(pin[name + "_params"], P)
    # tanh is numpy's here and the platform's numpy may round it differently: the fixture's dev_ref is a figure of the same size
    assert 0.25 * dev <= float(pin[key + "dev_ref"]) <= 4.0 * dev


# ---- 5. Newton on the restated Jacobian ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", vx.STAGES)
def test_newton_converges_from_every_start(name):
    import newton_reference as nr
    P, prob, z = setting(name)
    starts = vx.newton_starts(z, NEWTON_FACTOR)
    res = vx.newton_rows(P, SHIPPED, prob, starts)
    record("5 %s" % name, "factor %.0e, %d starts: status %s, iterations %s, halvings %s, max rnorm %.3e, spread of the roots %.3e"
           % (NEWTON_FACTOR, len(starts), [nr.STATUS_NAMES[s] for s in sorted(set(res["status"].tolist()))], res["iters"].tolist(),
              res["nhalf"].tolist(), res["rnorm"].max(), np.abs(res["z"] - res["z"][0]).max()))
    assert np.all(res["status"] == nr.CONVERGED)
    pin = np.load(os.path.join(GOLD, "vtol_exact_pin.npz"))
    assert float(pin["newton_factor"]) == NEWTON_FACTOR and np.array_equal(pin[name + "_newton_starts"], starts)
    assert np.all(np.abs(pin[name + "_newton_z"] - res["z"]) <= 1e-10 * np.maximum(1.0, np.abs(res["z"]))), "the fixture's roots"


# ---- 6. texts and symbols ------------------------------------------------------------------------------------------------------------

def test_texts_and_symbols():
    src = lambda *p: open(os.path.join(ROOT, *p)).read()          # noqa: E731
    dual, model, kern, impl = (src("socp_amd", "csrc", f) for f in ("dual.hpp", "models_vtol.hpp", "exact_jacobian.hpp", "plugin_impl.hpp"))
    assert "d_tanh(const Dual &a)" in dual and "(1.0 - th * th) * a.d" in dual
    import re
    assert not re.search(r"d_tanh", src("socp_amd", "csrc", "dualn.hpp")), "only Dual gets the rule"
    for text in ("control_t", "map_exact_t", "rhs_t", "hamiltonian_t", "switching_fn_t", "final_row_t", "switching_state_t",
                 "kSwitchingReadsXp = true", "kSwitchingStateXpContinuous = true"):
        assert text in model, text
    assert "has_final_row_t" in kern and "has_switching_state_t" in kern and "kSwitchingStateXpContinuous" in kern
    assert "exact_jacobian_covers_hooks" in impl
    make = src("socp_amd", "csrc", "Makefile")
    assert re.search(r"kernels_vtol_exact\.o:.*\n.*\n\t\$\(HIPCC\) \$\(COMMON\) \$\(EXACT_FLAGS\)", make), "built without contraction"
    for f in ("kernels_vtol.hip", "kernels_vtol_fast.hip"):
        t = src("socp_amd", "csrc", f)
        assert ", false>(VP_COUNT" in t and "t.fields = &fields_vtol" in t and "t.exact_jacobian = &exact_jacobian_vtol" in t
        assert not re.search(r"t\.(sensitivity|gain|gain_free|guide|hamiltonian_gradient|hamiltonian_jacobian|jacobi|events) =", t)
    header = src("include", "socp_hip.h")
    assert "d_tanh" in header and "kSwitchingStateXpContinuous" in header and "final_row_t" in header
    assert "int socp_ctx_set_exact_hooks(socp_ctx *ctx, int on);" in header and "socp_ctx_set_exact_hooks" in src("socp_amd", "csrc", "capi.cpp")
