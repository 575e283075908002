"""CPU: (a) the built library exports the singular-value entry points, capi wraps them and the sweep tool lists --sing-out; (b) the
definition of include/socp_hip.h as tests/svd_reference.py restates it: the schedule, the corner cases against hand-written answers,
and the accuracy against numpy.linalg.svd (LAPACK) on graded matrices and on the oracle's Jacobians.

The bound.  With unit = n eps sigma_max the three quantities
    r1 = max |sigma^ - sigma_LAPACK| / unit,   r2 = | ||A vmin||2 - sigma^_min | / unit,   r3 = | ||vmin||2 - 1 | / (n eps)
were MEASURED with the restatement (max_sweeps = 60) on U diag(s) V^T, s log-spaced over cond 2, 1e6, 1e12, n in {2, 3, 14, 15, 64,
65, 85, 127}: the largest r1 = 0.750 (n = 2, cond 1e6 and n = 64, cond 1e12), r2 = 0.242 (n = 64, cond 2), r3 = 0.250 (n = 2); and on
the oracle's Jacobians: Goddard n = 85 r1 = 0.392 unscaled / 0.555 scaled (r2 <= 1e-3, r3 = 0.012), double integrator n = 13
r1 = 0.044 / 0.190 (r3 = 0.038).  c = 4 x the largest ratio, rounded up = ceil(4 x 0.750) = 3 (LAPACK's own error is of the same
order, hence the factor); svd_reference.C_BOUND holds it for the GPU tests too.
Sweeps measured: <= 10 at cond 2, <= 23 at cond 1e6, <= 31 at cond 1e12; Goddard 11 unscaled / 15 scaled (sigma_min 3.36e-4,
cond 1.39e7 / 3.32e4); double integrator 3 / 5 (cond 2.47e6 / 5.45e3)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import svd_reference as sr
import tangent_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("socp_svd_batch_dev", "socp_singular_work_bytes", "socp_singular_batch_dev", "socp_singular_batch", "socp_singular_batch_blocks")
C = sr.C_BOUND


# ---- (a) ----------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_singular_value_entry_points_and_capi_wraps_them():
    from socp_amd import capi
    lib = ctypes.CDLL(capi.LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    for name in ("svd_batch_dev", "singular_batch", "singular_batch_dev", "singular_work_bytes"):
        assert callable(getattr(capi.Context, name, None)), name
    L = capi.lib()
    assert L.socp_singular_work_bytes.restype is ctypes.c_size_t and len(L.socp_singular_batch_blocks.argtypes) == 16
    assert len(L.socp_svd_batch_dev.argtypes) == 9 and len(L.socp_singular_batch_dev.argtypes) == 14
    # without a context nothing is sized
    assert L.socp_singular_work_bytes(None, 1) == 0


def test_sweep_tool_lists_sing_out_and_refuses_a_bad_scale():
    run = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert "--sing-out" in run.stdout and "--sing-scale" in run.stdout and "--sing-sweeps" in run.stdout
    # argument errors come before any device work: exit status 2 on a machine without a GPU too
    for extra, word in ((["--sing-scale", "2"], "--sing-scale"), (["--sing-sweeps", "0"], "--sing-sweeps"),
                        (["--sing-sweeps", "1001"], "--sing-sweeps"), (["--model", "interceptor"], "--sing-out")):
        bad = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--sing-out", "x"] + extra, cwd=ROOT, capture_output=True, text=True,
                             timeout=120)
        assert bad.returncode == 2 and word in bad.stderr, (extra, bad.stderr[-300:])


# ---- (b) ----------------------------------------------------------------------------------------------------------------------

def test_schedule_visits_every_pair_once_per_sweep_in_disjoint_steps():
    for n in range(1, 144):
        steps = sr.schedule(n)
        m = n + (n & 1)
        assert len(steps) == m - 1
        seen = []
        for pairs in steps:
            rows = [r for pq in pairs for r in pq]
            assert len(rows) == len(set(rows)), (n, "a step's pairs share a row")
            assert all(0 <= p < q < n for p, q in pairs)
            seen += pairs
        assert len(seen) == len(set(seen)) == n * (n - 1) // 2, n


def test_corner_cases_against_hand_written_answers():
    # n = 1: no pair, one sweep; the vector is +1 whatever the entry's sign
    r = sr.svd_batch(np.array([[-2.5], [0.0], [3.0]]))
    assert np.array_equal(r["sigma"], [[2.5], [0.0], [3.0]]) and np.array_equal(r["vt"].ravel(), [1.0, 0.0, 1.0])
    assert np.array_equal(r["sweeps"], [1, 1, 1]) and np.array_equal(r["info"], [0, 0, 0])
    # identity: no rotation, one sweep, Vt = I
    for n in (2, 5, 14):
        r = sr.svd_batch(np.eye(n).reshape(1, -1))
        assert r["sweeps"][0] == 1 and r["info"][0] == 0 and np.array_equal(r["sigma"][0], np.ones(n)) and np.array_equal(r["vt"][0], np.eye(n))
    # a permuted diagonal with signs: ordering (equal values by ascending row) and signs
    A, sigma, Vt = sr.permuted_diagonal()
    r = sr.svd_batch(A)
    assert r["sweeps"][0] == 1 and r["info"][0] == 0 and np.array_equal(r["sigma"][0], sigma) and np.array_equal(r["vt"][0], Vt)
    # the mixed batch: NaN / Inf -> info 2, sweeps 0, all NaN; the zero matrix; two equal rows
    n = 14
    A = sr.mixed_batch(n)
    r = sr.svd_batch(A)
    assert np.array_equal(r["info"], [0, 0, 2, 0, 2, 0, 0, 0]) and r["sweeps"][2] == r["sweeps"][4] == 0
    assert np.all(np.isnan(r["sigma"][[2, 4]])) and np.all(np.isnan(r["vt"][[2, 4]]))
    assert r["sweeps"][5] == 1 and np.all(r["sigma"][5] == 0.0) and np.all(r["vt"][5] == 0.0)
    assert r["sigma"][6, -1] <= C * n * sr.EPS * r["sigma"][6, 0], "two equal rows: sigma_min is zero or at noise level"
    assert r["sigma"][6, -2] > 1e-3 * r["sigma"][6, 0]
    healthy = [0, 1, 3, 7]
    assert np.all(r["sweeps"][healthy] >= 3) and np.all(np.diff(r["sigma"][healthy], axis=1) <= 0)
    # max_sweeps = 2 on a random n = 14 matrix: info 1, sweeps 2, the outputs from W as it stands (finite)
    r2 = sr.svd_batch(A[:1], max_sweeps=2)
    assert r2["info"][0] == 1 and r2["sweeps"][0] == 2 and np.all(np.isfinite(r2["sigma"])) and np.all(np.isfinite(r2["vt"]))
    # a row's result does not depend on its neighbours in the batch
    alone = sr.svd_batch(A[3:4])
    assert np.array_equal(alone["sigma"][0], r["sigma"][3]) and np.array_equal(alone["vt"][0], r["vt"][3])


@pytest.mark.parametrize("n", sr.SIZES)
def test_restatement_against_lapack_on_graded_matrices(n):
    A, r = sr.graded_reference(n)
    assert np.all(r["info"] == 0) and np.all(r["sweeps"] <= sr.MAX_SWEEPS)
    for k, cond in enumerate(sr.CONDS):
        q = sr.accuracy_ratios(A[k], r["sigma"][k], r["vt"][k, n - 1])
        print("n = %3d cond %.0e: sweeps %2d, ratios sigma %.3f, |A vmin| %.3f, |vmin| %.3f (bound c = %g)" % ((n, cond, r["sweeps"][k]) + q + (C,)))
        assert q[0] <= C and q[1] <= C and q[2] <= C, (n, cond, q)
        assert np.all(np.diff(r["sigma"][k]) <= 0)
        # the rows of Vt are orthonormal to the same level (not a bound of the issue: a sanity check of the vectors as a set)
        V = r["vt"][k]
        assert np.max(np.abs(V @ V.T - np.eye(n))) <= 50 * n * sr.EPS


@pytest.mark.parametrize("name", ["goddard", "dint"])
def test_oracle_jacobians_converge_agree_with_lapack_and_bound_the_tangent(name):
    c = tr.goddard_case() if name == "goddard" else tr.dint_case()
    o, prob, z = c["o"], c["prob"], np.asarray(c["Z"])[0]
    n = prob.n
    direction = (tr.DIR_PARAM, 0) if name == "goddard" else (tr.DIR_XNODE, 12)
    t = tr.tangent_reference(o, prob, c["nparams"], z[None, :], [direction])
    J = t["J"][0]                                                 # J[i][j]
    Jc = sr.colmajor(J)[None, :]
    smin = {}
    for scale in (0, 1):
        r = sr.singular_batch(Jc, scale, sr.MAX_SWEEPS)
        Js = sr.column_scale(Jc)[0] if scale else Jc
        q = sr.accuracy_ratios(Js[0], r["sigma"][0], r["vmin"][0])
        print("%s n = %d scale %d: sweeps %d, sigma_min %.3e, cond %.3e, ratios %.3f %.3f %.3f" % (
            (name, n, scale, r["sweeps"][0], r["sigma"][0, -1], r["sigma"][0, 0] / r["sigma"][0, -1]) + q))
        assert r["info"][0] == 0 and max(q) <= C, q
        if scale:
            assert np.array_equal(r["colnorm"][0], np.sqrt(sr.seq_dot(J.T, J.T)))
            assert np.allclose(np.linalg.norm(Js[0].reshape(n, n), axis=1), 1.0, rtol=0, atol=n * sr.EPS)
        else:
            assert np.all(r["colnorm"] == 1.0)
        smin[scale] = r["sigma"][0, -1]
    # J dz = -G, hence ||dz||2 <= ||G||2 / sigma_min
    dz, G = t["dz"][0, 0], t["fp"][0, 0]
    print("%s: ||dz|| = %.3e <= ||G|| / sigma_min = %.3e" % (name, np.linalg.norm(dz), np.linalg.norm(G) / smin[0]))
    assert t["info"][0] == 0 and np.linalg.norm(dz) <= np.linalg.norm(G) / smin[0]
