"""CPU: (a) the built library exports the tangent entry points and capi wraps them; (b) the conditions the GPU tests of
socp_tangent_batch rest on, on the CPU oracle with tests/tangent_reference.py: the tangent is a first-order predictor (its error
falls by four per halving of the move), the Goddard elimination pivots, every direction kind gives a finite tangent."""
import ctypes
import os
import subprocess
import sys

import numpy as np

import tangent_reference as tr
from tangent_reference import DIR_PARAM, DIR_TIME, DIR_XNODE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("socp_tangent_work_bytes", "socp_tangent_batch_dev", "socp_tangent_batch", "socp_tangent_batch_blocks", "socp_linsolve_batch_dev")


# ---- (a) ----------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_tangent_entry_points_and_capi_wraps_them():
    from socp_amd import capi
    lib = ctypes.CDLL(capi.LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    assert (capi.DIR_PARAM, capi.DIR_TIME, capi.DIR_XNODE) == (DIR_PARAM, DIR_TIME, DIR_XNODE) == (0, 1, 2)
    for name in ("tangent_batch", "tangent_batch_dev", "tangent_work_bytes", "linsolve_batch_dev"):
        assert callable(getattr(capi.Context, name, None)), name
    L = capi.lib()
    assert L.socp_tangent_work_bytes.restype is ctypes.c_size_t and len(L.socp_tangent_batch_blocks.argtypes) == 15
    # without a context nothing is sized
    assert L.socp_tangent_work_bytes(None, 1, 1) == 0


def test_sweep_tool_lists_tangent_out_and_refuses_an_unknown_parameter():
    run = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert "--tangent-out" in run.stdout and "--tangent-param" in run.stdout
    # argument errors come before any device work: exit status 2 on a machine without a GPU too
    bad = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--tangent-out", "x", "--tangent-param", "nosuch"], cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--tangent-param" in bad.stderr
    bad = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--model", "interceptor", "--tangent-out", "x"], cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--tangent-out" in bad.stderr


# ---- (b) ----------------------------------------------------------------------------------------------------------------------

def test_dint_tangent_in_the_target_is_a_first_order_predictor():
    """Case 1: the target Xf[0] (xnode entry 12) of the double integrator moved by 4 %, 2 %, 1 %."""
    from oracle.oracle import Problem
    c = tr.dint_case()
    o, prob, z0 = c["o"], c["prob"], c["Z"][0]
    ref = tr.tangent_reference(o, prob, 3, z0[None, :], [(DIR_XNODE, 12)])
    assert ref["info"][0] == 0
    theta = prob.xnode[1, 0]
    assert theta == 10.0

    def solve_at(value, start):
        X = prob.xnode.copy()
        X[1, 0] = value
        return tr.polished(o, Problem(prob.dim, prob.mode_t, prob.mode_x, prob.time, X), start)
    first, zero = tr.predictor_errors(solve_at, z0, ref["dz"][0, 0], theta, [0.04, 0.02, 0.01])
    tr.check_second_order(first, zero, "dint, Xf[0]")


def test_goddard_tangent_in_C_is_a_first_order_predictor_and_its_elimination_pivots():
    """Cases 2 and 3: parameter C (slot 0) of the stage-3 Goddard solution moved by 2 %, 1 %, 0.5 %; the elimination of its
    Jacobian swaps rows at least once, so the pivot search of the device kernel is exercised by the Goddard GPU case."""
    c = tr.goddard_case()
    o, prob, z0 = c["o"], c["prob"], c["Z"][0]
    ref = tr.tangent_reference(o, prob, 8, z0[None, :], [(DIR_PARAM, 0)])
    assert ref["info"][0] == 0 and ref["swaps"][0] >= 1, ref["swaps"]
    # the elimination agrees with LAPACK's to rounding level times the growth the condition number allows
    lapack = np.linalg.solve(ref["J"][0], -ref["fp"][0, 0])
    rel = np.max(np.abs(lapack - ref["dz"][0, 0])) / np.max(np.abs(lapack))
    print("goddard n = 85: cond(J) = %.2e, |dz - lapack| / |dz| = %.2e, row swaps %d" % (np.linalg.cond(ref["J"][0]), rel, ref["swaps"][0]))
    assert rel <= 1e-9
    theta = o.params()[0]
    own = o.params().copy()

    def solve_at(value, start):
        o.m.p[0] = value
        try:
            return tr.polished(o, prob, start)
        finally:
            o.set_params(own)
    first, zero = tr.predictor_errors(solve_at, z0, ref["dz"][0, 0], theta, [0.02, 0.01, 0.005])
    tr.check_second_order(first, zero, "goddard, C")


def test_every_direction_kind_gives_a_finite_tangent():
    """Case 4.  The time of the FREE end node and an ignored parameter slot are not refused: G = 0, dz = -+0."""
    c = tr.dint_case()
    dirs = [(DIR_PARAM, 1), (DIR_PARAM, 2), (DIR_TIME, 0), (DIR_XNODE, 1), (DIR_XNODE, 12), (DIR_TIME, 1), (DIR_PARAM, 4)]
    ref = tr.tangent_reference(c["o"], c["prob"], 3, c["Z"], dirs)
    assert np.all(ref["info"] == 0) and np.all(np.isfinite(ref["dz"])) and np.all(np.isfinite(ref["fp"]))
    assert np.all(np.max(np.abs(ref["dz"][:, :5]), axis=2) > 0), "the directions the residual reads move the solution"
    assert np.all(ref["fp"][:, 5:] == 0) and np.all(ref["dz"][:, 5:] == 0), "a FREE node's time and a switching-time slot are not read"
    g = tr.goddard_case()
    dirs = [(DIR_PARAM, 2), (DIR_PARAM, 6), (DIR_TIME, 0), (DIR_XNODE, 0), (DIR_XNODE, 6 * 14)]
    ref = tr.tangent_reference(g["o"], g["prob"], 8, g["Z"], dirs)
    assert ref["info"][0] == 0 and np.all(np.isfinite(ref["dz"])) and np.all(np.max(np.abs(ref["dz"][0]), axis=1) > 0)


def test_elimination_failures_and_ties():
    """The restatement's own corner cases: lowest index among equal pivots, singular -> k + 1 and NaN rows, NaN / infinite entries."""
    X, info, swaps = tr.eliminate([[1.0, 2.0], [-1.0, 1.0]], [[3.0, 0.0]])
    assert info == 0 and swaps == 0 and np.array_equal(X, [[1.0, 1.0]])
    X, info, _ = tr.eliminate([[1.0, 2.0], [2.0, 4.0]], [[1.0, 1.0], [0.0, 1.0]])
    assert info == 2 and X.shape == (2, 2) and np.all(np.isnan(X))
    assert tr.eliminate([[np.nan, 1.0], [1.0, 1.0]], [[1.0, 1.0]])[1] == 1, "a NaN on the diagonal stays: no pivot"
    assert tr.eliminate([[1.0, 1.0], [np.nan, 1.0]], [[1.0, 1.0]])[1] == 2, "a NaN below it is not chosen and poisons the next step"
    assert tr.eliminate([[np.inf, 1.0], [1.0, 1.0]], [[1.0, 1.0]])[1] == 1
    assert tr.eliminate([[1.0, 0.0], [0.0, 1.0]], [[np.inf, 1.0]])[1] == 3, "only a solution entry is not finite: n + 1"
