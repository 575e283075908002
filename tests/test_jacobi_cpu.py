"""CPU: the definition of socp_jacobi_batch as tests/jacobi_reference.py restates it -- the determinant against numpy, and the whole
instrument on two models with closed-form Jacobi fields (the example plugins' right-hand sides, RK4 restated).  Every check is a
function of the restatement it is given, so that the last test can hand it a corrupted one and see it fail.  No GPU."""
import ctypes
import math

import numpy as np
import pytest

import jacobi_reference as jr

U = 2.0 ** -53                                   # unit roundoff
DIMS = (1, 2, 3, 6, 7)


# ---- 0. the symbols ---------------------------------------------------------------------------------------------------------

def test_library_exports_the_jacobi_entry_points():
    from socp_amd import capi
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in ("socp_jacobi_batch", "socp_jacobi_batch_dev", "socp_jacobi_batch_blocks", "socp_ctx_has_jacobi"):
        assert hasattr(lib, name), name


# ---- 1. the determinant ---------------------------------------------------------------------------------------------------

def pivots(A):
    """The pivots of Gaussian elimination with partial pivoting, vectorised (only to size numpy's own error below)."""
    a = np.array(A, dtype=np.float64)
    out = []
    for k in range(a.shape[0]):
        p = k + int(np.argmax(np.abs(a[k:, k])))
        a[[k, p]] = a[[p, k]]
        out.append(a[k, k])
        if a[k, k] != 0.0:
            a[k + 1:] -= np.outer(a[k + 1:, k] / a[k, k], a[k])
    return np.array(out)


def det_tolerance(A, against_numpy=True):
    """Gaussian elimination with partial pivoting computes the exact factors of A + E with |E| <= gamma_D |L| |U| (Higham, Accuracy
    and Stability of Numerical Algorithms, Thm 9.3), |L| <= 1 and max |U| <= rho max |A| with the growth factor rho <= 2^(D-1): a
    column of E is at most D gamma_D 2^(D-1) times its own column's norm once the columns are scaled to equal norms, which changes
    neither a pivot choice nor a relative error.  By multilinearity and Hadamard's inequality, to first order
    |det(A + E) - det A| <= (sum over the columns of ||E_j|| / ||A_j||) prod ||A_j|| <= D * D gamma_D 2^(D-1) prod ||A_j||, and the
    product of the D pivots adds D u.  Twice that, because numpy's LAPACK factorisation is the same algorithm with its own roundings;
    and numpy forms the determinant as sign * exp(sum of log |pivot|), whose relative error is the absolute error of that sum:
    u (|log| + 1) per pivot, u per addition, and the exp's own -- 2 u (sum |log |pivot|| + 2 D + 2) |det| more."""
    D = A.shape[0]
    gamma = D * U / (1.0 - D * U)
    tol = 2.0 * (D * D * gamma * 2.0 ** (D - 1) + D * U) * float(np.prod(np.linalg.norm(A, axis=0)))
    if against_numpy:
        pv = np.abs(pivots(A))
        logs = float(np.sum(np.abs(np.log(pv[pv > 0.0]))))
        tol += 2.0 * U * (logs + 2.0 * D + 2.0) * abs(float(np.linalg.det(A)))
    return tol


def general_matrices(D, rng):
    """Random ones, and pivot-forcing ones: the largest entry of every column at the bottom, a reversed identity plus noise."""
    out = [rng.standard_normal((D, D)) * 10.0 ** rng.uniform(-3, 3, size=(1, D)) for _ in range(20)]
    for _ in range(10):
        A = rng.standard_normal((D, D))
        A *= np.arange(1, D + 1, dtype=np.float64)[:, None] ** 2
        out.append(A)
        out.append(np.eye(D)[::-1] * 5.0 + 0.1 * rng.standard_normal((D, D)))
    return out


def integer_matrices(D, rng):
    """Row-permuted upper-triangular integer matrices: every column has ONE nonzero among the rows still in play, so every multiplier
    is 0, every operation exact and the determinant sign(P) prod T_kk -- exactly, in any elimination order."""
    out = []
    for _ in range(30):
        T = np.triu(rng.integers(-9, 10, size=(D, D))).astype(np.float64)
        T[np.arange(D), np.arange(D)] = rng.choice([-7, -3, -2, -1, 1, 2, 3, 5, 8], size=D)
        perm = rng.permutation(D)
        inversions = sum(1 for i in range(D) for j in range(i + 1, D) if perm[i] > perm[j])
        out.append((T[perm], float(np.prod(np.diag(T))) * (-1.0 if inversions % 2 else 1.0), inversions))
    return out


def check_determinant(det):
    """det(J) -> (value, swaps): the restatement under test."""
    rng = np.random.default_rng(20251019)
    odd = 0
    for D in DIMS:
        for A in general_matrices(D, rng):
            got, swaps = det(A)
            assert abs(got - np.linalg.det(A)) <= det_tolerance(A), (D, got, np.linalg.det(A), det_tolerance(A))
            odd += swaps % 2
        for A, want, inversions in integer_matrices(D, rng):
            got, swaps = det(A)
            assert got == want and got == round(np.linalg.det(A)), (D, got, want)
            assert swaps % 2 == inversions % 2
    assert odd >= 10, "the matrices force row swaps"
    # the special values
    assert math.isnan(det(np.array([[1.0, np.inf], [0.0, 1.0]]))[0]) and math.isnan(det(np.array([[np.nan]]))[0])
    z = det(np.array([[1.0, 2.0], [2.0, 4.0]]))[0]
    assert z == 0.0 and not math.copysign(1.0, z) < 0, "a zero pivot: +0.0"
    assert det(np.zeros((3, 3)))[0] == 0.0


def test_determinant_of_the_restatement_agrees_with_numpy():
    check_determinant(jr.det_reference)


# ---- 2. osc1d: conjugate times k pi / sqrt(w) ---------------------------------------------------------------------------------

OSC = dict(w=4.0, T=4.0, N=400, X0=np.array([0.3, 0.7]))


def osc_bound(t_star, skip_steps=0):
    """|tconj - t*| for the oscillator, omega = sqrt(w) = 2, h = T / N = 0.01, J(t) = -sin(omega t) / omega, |J'(t*)| = 1:
      truncation     RK4 on a linear oscillator turns the phase by omega h (1 - (omega h)^4 / 120 + ...) per step: after t the field is off
                     by at most t omega^4 h^4 / 120 (amplitude errors are O(h^5) per unit time); doubled for the higher terms
      interpolation  linear interpolation over one step: h^2 / 8 max |J''|, and |J''| = omega |sin(omega t)| <= omega * omega h within
                     a step of the root:  omega^2 h^3 / 8
      quotient       each trajectory carries the roundings of k = t / h steps; per step and component the update X + h6 (...) rounds
                     once at the size of X (|X| <= 1) and the stage arithmetic adds terms h omega times smaller: <= 2 u; the
                     flow moves an error between x and p with a factor <= omega: 2 omega k u per trajectory, two trajectories,
                     divided by h_c = eps |p0|
    each divided by the smallest slope over the bracketing step, cos(omega h)."""
    w, T, N, X0 = OSC["w"], OSC["T"], OSC["N"], OSC["X0"]
    om, h = math.sqrt(w), T / N
    k = math.ceil(t_star / h) + 1
    hc = jr.fd_eps(0.0) * abs(X0[1])
    trunc = 2.0 * t_star * om ** 4 * h ** 4 / 120.0
    interp = om ** 2 * h ** 3 / 8.0
    quot = 2.0 * (2.0 * om * k * U) / hc
    return (trunc + interp + quot) / math.cos(om * h)


def check_osc1d(segment):
    w, T, N, X0 = OSC["w"], OSC["T"], OSC["N"], OSC["X0"]
    step = jr.rk4_of(jr.osc1d_rhs(w))
    s = segment(step, 1, 0.0, T, X0, N, jr.fd_eps(0.0), stride=1, skip=0)
    assert s["count"] == N and s["nchange"] == 2
    b = osc_bound(math.pi / 2)
    print("osc1d: tconj - pi/2 = %.3e (bound %.3e)" % (s["tconj"] - math.pi / 2, b))
    assert abs(s["tconj"] - math.pi / 2) <= b
    assert b < 2e-5, "the bound says something"
    # skip behind the first conjugate time: only the second one is seen
    s2 = segment(step, 1, 0.0, T, X0, N, jr.fd_eps(0.0), stride=1, skip=200)
    assert s2["nchange"] == 1 and abs(s2["tconj"] - math.pi) <= osc_bound(math.pi)
    # w = 0: J = -t, no conjugate time
    s0 = segment(jr.rk4_of(jr.osc1d_rhs(0.0)), 1, 0.0, T, X0, N, jr.fd_eps(0.0), stride=1, skip=0)
    assert s0["nchange"] == 0 and math.isnan(s0["tconj"]) and all(d < 0.0 for d in s0["det"])


def test_osc1d_conjugate_time():
    check_osc1d(jr.jacobi_segment)


# ---- 3. lqr1d: det J(t) = g^2 t^4 / 12 -------------------------------------------------------------------------------------------

LQR = dict(g=1.0, T=2.0, N=40, X0=np.array([0.2, -0.3, 0.8, 0.6]), skip=2)


def lqr_bound(t, k):
    """|det - g^2 t^4 / 12| after k steps.  The solution is a cubic in t and RK4 integrates it without truncation error, the flow is
    linear in the costate, so the difference quotient has no O(h_c) term: what is left is rounding.
      per trajectory   <= 3 u |X|max per step and component (the update's rounding at the size of X, the stage terms h times smaller),
                       |X|max <= 1.2 on [0, 2] for this start; an error moves down the chain p_x -> p_v -> v -> x with factors
                       1, t, t^2/2, t^3/6 (their sum <= 6.4 for t <= 2):  e = 6.4 * 3 * 1.2 * k u
      per entry of J   dJ = 2 e / min h_c
      determinant      |det(J + dJ) - det J| <= dJ * sum |J_ij| + 2 dJ^2 for a 2 x 2 matrix, J = g [[t^3/6, -t^2/2], [t^2/2, -t]]
      elimination      det_tolerance's bound for D = 2 against the product of the column norms."""
    g, X0 = LQR["g"], LQR["X0"]
    e = 6.4 * 3.0 * 1.2 * k * U
    dJ = 2.0 * e / (jr.fd_eps(0.0) * min(abs(X0[2]), abs(X0[3])))
    J = g * np.array([[t ** 3 / 6.0, -t ** 2 / 2.0], [t ** 2 / 2.0, -t]])
    return dJ * float(np.abs(J).sum()) + 2.0 * dJ * dJ + det_tolerance(J, against_numpy=False)


def check_lqr1d(segment):
    g, T, N, X0, skip = LQR["g"], LQR["T"], LQR["N"], LQR["X0"], LQR["skip"]
    s = segment(jr.rk4_of(jr.lqr1d_rhs(g)), 2, 0.0, T, X0, N, jr.fd_eps(0.0), stride=1, skip=skip)
    assert s["count"] == N
    worst = 0.0
    for j in range(skip, N):
        t, want = s["tq"][j], g * g * s["tq"][j] ** 4 / 12.0
        b = lqr_bound(t, j + 1)
        assert b < want, "skip and the horizon keep the bound below the determinant at every compared sample"
        assert abs(s["det"][j] - want) <= b, (j, s["det"][j], want, b)
        worst = max(worst, abs(s["det"][j] - want) / b)
    print("lqr1d: largest |det - g^2 t^4 / 12| / bound = %.3e" % worst)
    assert s["nchange"] == 0 and math.isnan(s["tconj"])
    want_J = g * np.array([[T ** 3 / 6.0, -T ** 2 / 2.0], [T ** 2 / 2.0, -T]])
    assert np.max(np.abs(s["jend"] - want_J)) <= 2.0 * (6.4 * 3.0 * 1.2 * N * U) / (jr.fd_eps(0.0) * 0.6)


def test_lqr1d_determinant():
    check_lqr1d(jr.jacobi_segment)


# ---- 4. the checks reject corrupted restatements -----------------------------------------------------------------------------

def test_corrupted_restatements_fail():
    with pytest.raises(AssertionError):
        check_determinant(lambda A: jr.det_reference(A, swap_sign=False))
    with pytest.raises(AssertionError):
        check_lqr1d(lambda *a, **k: jr.jacobi_segment(*a, swap_sign=False, **k))
    with pytest.raises(AssertionError):
        check_osc1d(lambda *a, **k: jr.jacobi_segment(*a, use_skip=False, **k))
