"""CPU: the definition of socp_fields_batch as tests/fields_reference.py restates it -- (a) the restated right-hand sides against the
oracle, bit for bit; (b) the dual-number rules against central differences of the same text in 240 bits; (c) the value part against
the oracle's RK4 trajectory, bit for bit; (d) the accuracy of the exact fields against the 240-bit dual recurrence, measured beside
the forward difference of socp_jacobi_batch; (e) the whole transition matrix against the reference's own variational equations;
(f) the instrument: corrupted restatements must fail.  No GPU; the library is only asked for its symbols.

Measured (profiles/fields_cpu_tests.txt), deviation of Jend from the 240-bit recurrence, max-norm, exact / forward difference:
Goddard mu2 = 1: 5.8e-11 / 2.5e-2 (ratio 2.3e-9), mu2 = 0.2: 1.6e-13 / 3.3e-4 (4.8e-10), mu2 = 0 with sw = (0.05, 0.15): 2.1e-13 / 3.1e-4
(6.6e-10); covid19 3.9e-11, the saturated double integrator 6.0e-11; the bar is 1e-6.  (e): 4.0e-15 on both sides."""
import math

import numpy as np
import pytest

import fields_reference as fr
import jacobi_reference as jr
from conftest import GODDARD_X0_STATE, GODDARD_PSTAR

pytestmark = pytest.mark.skipif(not fr.HAVE_MPMATH, reason="mpmath is the 240-bit carrier")

TF = 0.2640825
N = 50
X0_GODDARD = np.concatenate([GODDARD_X0_STATE, GODDARD_PSTAR])
GODDARD_SETTINGS = {"mu2=1": (1.0, (0.0, 0.0)), "mu2=0.2": (0.2, (0.0, 0.0)), "mu2=0": (0.0, (0.05, 0.15))}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def goddard_oracle(mu2, sw, n=N):
    from oracle.oracle import Oracle, MODEL_GODDARD
    o = Oracle(MODEL_GODDARD, step_nbr=n)
    o.set_param("mu2", mu2)
    o.set_switching(list(sw))
    return o


def covid_oracle(n=N):
    from oracle.oracle import Oracle, MODEL_COVID
    o = Oracle(MODEL_COVID, step_nbr=n)
    o.m.p[0], o.m.p[1], o.m.p[2] = 3.4, 14.0, 5.0
    return o


def dint_oracle(n=N):
    from oracle.oracle import Oracle, MODEL_DINT
    return Oracle(MODEL_DINT, step_nbr=n)


X0_COVID = np.array([0.93, 0.003, 0.01, 0.057, -0.001, 0.001, 0.0, 0.0])
X0_DINT = np.array([0.0, 0.0, 0.0, 0.3, -0.2, 0.1, 0.02, -0.01, 0.015, 0.4, -0.3, 0.2])      # |u| = 0.54 < u_max = 1
X0_DINT_SAT = np.array([0.0, 0.0, 0.0, 0.3, -0.2, 0.1, 0.02, -0.01, 0.015, 2.0, -1.5, 1.0])   # |u| = 2.7: saturated all along


# ---- (a) the restated right-hand sides equal the oracle's, bit for bit --------------------------------------------------------

def goddard_rows(rng, count, sw):
    X = np.tile(X0_GODDARD, (count, 1)) * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, size=(count, 14)))
    X[:, 3:6] = rng.uniform(-0.05, 0.05, size=(count, 3)) * rng.choice([1e-9, 1.0], size=(count, 1))
    t = rng.uniform(0.0, 0.2, size=count)                   # sw = (0.05, 0.15): all three arcs
    return X, t


@pytest.mark.parametrize("setting", list(GODDARD_SETTINGS))
def test_a_goddard_restatement_equals_the_oracle(setting):
    mu2, sw = GODDARD_SETTINGS[setting]
    o = goddard_oracle(mu2, sw)
    P = o.params()[:8]
    X, t = goddard_rows(np.random.default_rng(11), 600, sw)
    arcs = set()
    for k in range(600):
        assert np.array_equal(bits(o.rhs(t[k], X[k])), bits(fr.plain_rhs("goddard", P, sw, t[k], X[k]))), k
        arcs.add(0 if t[k] <= sw[0] else (1 if t[k] <= sw[1] else 2))
    if mu2 == 0.0:
        assert arcs == {0, 1, 2} and P[7] < 0             # the singular arc with the closed-form control


def test_a_covid_restatement_equals_the_oracle():
    o = covid_oracle()
    P = o.params()[:8]
    rng = np.random.default_rng(12)
    seen = set()
    for k in range(600):
        X = np.concatenate([rng.uniform(0.0, 1.0, 4) * [1.0, 0.05, 0.3, 0.3], rng.uniform(-1.0, 1.0, 4) * rng.choice([0.01, 1e3])])
        K = fr.PlainKit()
        ref = np.array(fr.rhs_on(fr.covid_ref, K, [float(p) for p in P], [0.0, 0.0], 0.0, [float(x) for x in X]))
        assert np.array_equal(bits(o.rhs(0.0, X)), bits(ref)), k
        seen |= {n for n, m in K.margins.items() if (m <= 0 if n == "u-umin" else m >= 0)}
    assert seen == {"u-umin", "u-umax", "I-Imax"}             # both clamps and the penalty were active somewhere


def test_a_dint_restatement_equals_the_oracle():
    o = dint_oracle()
    P = o.params()[:3]
    rng = np.random.default_rng(13)
    sat = 0
    for k in range(600):
        X = rng.uniform(-1.0, 1.0, 12) * rng.choice([0.3, 3.0])
        assert np.array_equal(bits(o.rhs(0.0, X)), bits(fr.plain_rhs("dint", P, (0.0, 0.0), 0.0, X))), k
        sat += math.sqrt(sum((X[9:] / P[1]) ** 2)) > P[0]
    assert 50 < sat < 550


# ---- (b) the derivative rules against central differences of the same text, 240 bits -------------------------------------------

def dual_jacobian_mpf(model, P, sw, t, X, cls=None):
    cls = cls or fr.DualMpf
    mp = fr.mpf
    S = len(X)
    Pn, swn, tn = [mp(float(p)) for p in P], [mp(float(s)) for s in sw], mp(float(t))
    cols, margins = [], {}
    for k in range(S):
        K = fr.DualMpfKit()
        d = fr.rhs_on(fr.RHS[model], K, Pn, swn, tn, [cls(mp(float(X[j])), mp(1.0 if j == k else 0.0)) for j in range(S)])
        cols.append([q.d if isinstance(q, fr.Dual) else mp(0.0) for q in d])
        margins = K.margins
    return cols, margins


def central_jacobian_mpf(model, P, sw, t, X, h):
    mp = fr.mpf
    S = len(X)
    Pn, swn, tn = [mp(float(p)) for p in P], [mp(float(s)) for s in sw], mp(float(t))
    f = lambda Y: fr.rhs_on(fr.RHS[model], fr.MpfKit(), Pn, swn, tn, Y)   # noqa: E731
    cols = []
    for k in range(S):
        Xp = [mp(float(X[j])) + (h if j == k else 0) for j in range(S)]
        Xm = [mp(float(X[j])) - (h if j == k else 0) for j in range(S)]
        cols.append([(a - b) / (2 * h) for a, b in zip(f(Xp), f(Xm))])
    return cols


def derivative_rows():
    """Rows away from every kink (margins >= 1e-6, against h = 1e-24) and of moderate size, so that h^2 f''' / 6 ~ 1e-48."""
    rng = np.random.default_rng(21)
    rows = []
    for setting, (mu2, sw) in GODDARD_SETTINGS.items():
        P = goddard_oracle(mu2, sw).params()[:8]
        for t in (0.02, 0.1, 0.18):
            X = np.concatenate([[1.0, 0.1, 0.2], rng.uniform(0.02, 0.08, 3), [0.9], rng.uniform(-1.0, 1.0, 7)])
            rows.append(("goddard", P, sw, t, X))
    Pc = covid_oracle().params()[:8]
    for scale in (0.01, 1e3):
        rows.append(("covid", Pc, (0.0, 0.0), 0.0, np.concatenate([[0.9, 0.01, 0.2, 0.05], rng.uniform(-1.0, 1.0, 4) * scale])))
    Pd = dint_oracle().params()[:3]
    rows.append(("dint", Pd, (0.0, 0.0), 0.0, X0_DINT))
    rows.append(("dint", Pd, (0.0, 0.0), 0.0, X0_DINT_SAT))
    return rows


def rule_deviation(cls=None):
    """The largest deviation between the dual derivative and the central difference over the rows, relative to the row's largest
    entry; the margins of every decision are checked against the step."""
    h = fr.mpf(10) ** -24
    worst = fr.mpf(0)
    for model, P, sw, t, X in derivative_rows():
        dual, margins = dual_jacobian_mpf(model, P, sw, t, X, cls)
        for name, m in margins.items():
            mv = m.v if isinstance(m, fr.Dual) else m
            assert abs(mv) > 1e-6, (model, name, mv)            # decidable: no kink within h
        cen = central_jacobian_mpf(model, P, sw, t, X, h)
        big = max(abs(q) for col in cen for q in col)
        worst = max(worst, max(abs(a - b) for ca, cb in zip(dual, cen) for a, b in zip(ca, cb)) / big)
    return worst


def test_b_dual_rules_are_the_derivative():
    """Truncation h^2 f'''/6 and rounding 2^-240 / h are both ~ 1e-48 of the entries: 1e-40 is derived, not measured."""
    worst = rule_deviation()
    print("dual rules vs central difference, 240 bits: %.3e of the largest entry" % float(worst))
    assert worst <= fr.mpf(10) ** -40


# ---- (c) the value part is the oracle's trajectory, bit for bit ----------------------------------------------------------------

def oracle_trajectory(o, t1, t2, X0, n):
    """The residual's loop (jacobi_reference.jacobi_segment) on Oracle.rk4_step."""
    out = []
    X = np.array(X0, dtype=np.float64)
    dt = (t2 - t1) / n
    t, guard = t1, n + 8
    act = t < (t2 - dt / 2) and guard > 0
    while act:
        guard -= 1
        h = (t2 - t) if (t + dt > t2) else dt
        X = o.rk4_step(t, X, h)
        out.append(X.copy())
        t = t + dt
        act = t < (t2 - dt / 2) and guard > 0
    return out


def segments():
    """name -> (model, oracle, P, sw, D, t1, t2, X0): the segments of (c) and (d)."""
    out = {}
    for setting, (mu2, sw) in GODDARD_SETTINGS.items():
        o = goddard_oracle(mu2, sw)
        out["goddard " + setting] = ("goddard", o, o.params()[:8], sw, 7, 0.0, TF, X0_GODDARD)
    o = covid_oracle()
    out["covid"] = ("covid", o, o.params()[:8], (0.0, 0.0), 4, 0.0, 30.0, X0_COVID)
    # the unsaturated double integrator is linear: a forward difference has no truncation error there and the comparison of (d)
    # would say nothing, so (d) takes the saturated segment; (e) takes the unsaturated one
    o = dint_oracle()
    out["dint saturated"] = ("dint", o, o.params()[:3], (0.0, 0.0), 6, 0.0, 2.0, X0_DINT_SAT)
    return out


_SEG = {}


def segment_results(name):
    """(exact fields in doubles, the 240-bit recurrence, the forward difference of socp_jacobi_batch), computed once."""
    if name not in _SEG:
        model, o, P, sw, D, t1, t2, X0 = segments()[name]
        traj = []
        ex = fr.fields_segment(model, P, sw, D, t1, t2, X0, N, stride=7, trajectory=traj)
        hi = fr.fields_segment(model, P, sw, D, t1, t2, X0, N, cls=fr.DualMpf, kit=fr.DualMpfKit())
        fd = jr.jacobi_segment(lambda t, X, h: o.rk4_step(t, X, h), D, t1, t2, X0, N, jr.fd_eps(0.0), stride=7)
        _SEG[name] = (ex, hi, fd, traj)
    return _SEG[name]


@pytest.mark.parametrize("name", list(segments()))
def test_c_value_part_is_the_oracle_trajectory(name):
    model, o, P, sw, D, t1, t2, X0 = segments()[name]
    traj = segment_results(name)[3]
    ref = oracle_trajectory(o, t1, t2, X0, N)
    assert len(ref) == len(traj) == N
    for k in range(N):
        assert np.array_equal(bits(ref[k]), bits(traj[k])), k


# ---- (d) accuracy against the 240-bit dual recurrence, beside the forward difference ---------------------------------------------

def jend_deviation(J, truth):
    return max(abs(fr.mpf(float(J[r][c])) - truth[r][c]) for r in range(len(truth)) for c in range(len(truth)))


@pytest.mark.parametrize("name", list(segments()))
def test_d_exact_fields_against_the_240_bit_recurrence(name):
    D = segments()[name][4]
    ex, hi, fd, _ = segment_results(name)
    truth = fr.jend_of(hi["phi"], D)
    dev_exact = jend_deviation(fr.jend_of(ex["phi"], D), truth)
    dev_fd = jend_deviation(fd["jend"], truth)
    big = max(abs(q) for row in truth for q in row)
    det_truth = fr.mpmath.det(fr.mpmath.matrix(truth))
    print("%-16s max|J| %.3e  exact %.3e  forward difference %.3e  ratio %.3e  det truth %.6e  exact %.11e  fd %.6e"
          % (name, float(big), float(dev_exact), float(dev_fd), float(dev_exact / dev_fd), float(det_truth), ex["det"][-1], fd["det"][-1]))
    assert dev_exact <= fr.mpf(10) ** -6 * dev_fd


# ---- (e) the whole transition matrix against the reference's variational equations ------------------------------------------------

def test_e_transition_matrix_against_the_variational_equations():
    o = dint_oracle()
    P, S = o.params()[:3], 12
    t2 = 3.0
    ex = fr.fields_segment("dint", P, (0.0, 0.0), 6, 0.0, t2, X0_DINT, N, cols=fr.ALL)
    hi = fr.fields_segment("dint", P, (0.0, 0.0), 6, 0.0, t2, X0_DINT, N, cols=fr.ALL, cls=fr.DualMpf, kit=fr.DualMpfKit())
    Y = o.traj(0.0, np.concatenate([X0_DINT, np.eye(S).ravel()]), t2, is_jac=1)
    var = Y[S:].reshape(S, S)                               # R[k][i] at Y[S (k + 1) + i]
    dev = lambda A: max(abs(fr.mpf(float(A[r][c])) - hi["phi"][r][c]) for r in range(S) for c in range(S))   # noqa: E731
    d_exact, d_var = dev(ex["phi"]), dev(var)
    print("dint transition matrix against the 240-bit recurrence: dual numbers %.3e, variational equations %.3e" % (float(d_exact), float(d_var)))
    assert d_exact <= 8 * d_var and d_var <= 8 * d_exact


# ---- (f) the instrument ---------------------------------------------------------------------------------------------------------

def test_f_without_the_zero_rule_the_thrust_off_field_is_lost():
    """Goddard mu2 = 1 starts with the thrust off: norm_u = sqrt(0), whose derivative without the s == 0 rule is 0 / 0."""
    model, o, P, sw, D, t1, t2, X0 = segments()["goddard mu2=1"]
    good = segment_results("goddard mu2=1")[0]
    bad = fr.fields_segment(model, P, sw, D, t1, t2, X0, N, cls=fr.DualNoZeroRule)
    assert np.isfinite(good["phi"]).all() and not np.isfinite(bad["phi"]).all()


def test_f_a_product_rule_with_one_term_dropped_fails_b():
    class HalfMpf(fr.DualMpf):
        __slots__ = ()
        PRODUCT_BOTH_TERMS = False
    assert rule_deviation(HalfMpf) > fr.mpf(10) ** -40


def test_f_the_determinant_needs_the_swap_sign():
    """The determinant of the exact J against mpmath's of the 240-bit J: the sign and six digits, on a segment whose elimination
    swaps rows an odd number of times; without the swap sign the same check fails."""
    found = 0
    o = dint_oracle()
    short = ("dint", o.params()[:3], (0.0, 0.0), 6, 0.0, 2.0, X0_DINT, 20)      # dv/dp ~ t^2/2 outweighs dx/dp ~ t^3/6: rows are swapped
    pairs = [(n,) + segment_results(n)[:2] + (segments()[n][4],) for n in segments()]
    pairs.append(("dint short", fr.fields_segment(*short), fr.fields_segment(*short, cls=fr.DualMpf, kit=fr.DualMpfKit()), 6))
    for name, ex, hi, D in pairs:
        J = np.array(fr.jend_of(ex["phi"], D))
        truth = fr.mpmath.det(fr.mpmath.matrix(fr.jend_of(hi["phi"], D)))
        det, swaps = jr.det_reference(J)
        scale = float(np.prod(np.abs(J).max(axis=0)))
        if abs(float(truth)) <= 1e-6 * scale:                # zero to rounding: no sign to read
            continue
        assert abs(det - float(truth)) <= 1e-6 * abs(float(truth)), name
        if swaps % 2 == 1:
            found += 1
            wrong, _ = jr.det_reference(J, swap_sign=False)
            assert not abs(wrong - float(truth)) <= 1e-6 * abs(float(truth)), name
    assert found >= 1


def test_library_has_the_entry_points():
    """Fails without the feature: the C-ABI exports the four functions and the Python layer binds them."""
    from socp_amd import capi
    L = capi.lib()
    for name in ("socp_ctx_has_fields", "socp_fields_batch_dev", "socp_fields_batch", "socp_fields_batch_blocks"):
        assert hasattr(L, name), name
    assert capi.FIELDS_COSTATE == 0 and capi.FIELDS_ALL == 1
    for name in ("has_fields", "fields_batch_dev", "fields_batch"):
        assert callable(getattr(capi.Context, name))
