"""The inputs of the Jacobi-field tests and their CPU references (helper of test_gpu_jacobi_batch.py, not a test).  Every case is
built from the CPU oracle (or, for the two example plugins, from their restated right-hand sides) alone, so the coverage the GPU
tests rest on -- row swaps, slabs with and without a sign change -- is a property of the restatement's own output and can be
looked at without a GPU.  A case's reference is computed once per setting and shared read-only."""
import json
import os

import numpy as np

import jacobi_reference as jr
from conftest import GODDARD_X0_STATE, GODDARD_PSTAR, goddard_single_problem, goddard_costate_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
N_STEPS = 60


def perturbed(z, B, rel, seed):
    rng = np.random.default_rng(seed)
    Z = np.tile(np.asarray(z, dtype=np.float64), (B, 1))
    Z[1:] *= 1.0 + rel * rng.uniform(-1.0, 1.0, size=(B - 1, Z.shape[1]))
    return Z


def goddard_oracle(N=N_STEPS):
    from oracle.oracle import Oracle, MODEL_GODDARD
    o = Oracle(MODEL_GODDARD, step_nbr=N)
    o.set_param("mu2", 1.0)
    return o


def goddard_single():
    """BASELINE config 2: single shooting, fixed tf; 9 rows = 9 slabs at 8 groups per wave."""
    o = goddard_oracle()
    prob, _ = goddard_single_problem()
    return dict(model="goddard", o=o, prob=prob, N=N_STEPS, Z=goddard_costate_batch(9, 1e-2), params=o.params()[:8])


def goddard_m3(times=None, free_tf=True, B=9, seed=7):
    """M = 3 on the nominal trajectory over [0, 0.09], the costates of every node moved by 1 %; free tf (the last unknown).  27 slabs."""
    from oracle.oracle import Problem, FIXED, FREE, CONTINUOUS
    o = goddard_oracle()
    M, tf = 3, 0.09
    time = np.array([i * tf / M for i in range(M + 1)]) if times is None else np.asarray(times, dtype=np.float64)
    Xi = np.concatenate([GODDARD_X0_STATE, GODDARD_PSTAR])
    nodes = np.stack([Xi] + [o.traj(0.0, Xi, i * tf / M) for i in range(1, M)])
    mode_t = [FIXED, CONTINUOUS, CONTINUOUS, FREE] if free_tf else [FIXED] * (M + 1)
    mode_x = np.zeros((M + 1, 7), dtype=np.int32)
    mode_x[1:M] = CONTINUOUS
    mode_x[M, 3:7] = FREE
    X = np.zeros((M + 1, 14))
    X[0, :7] = GODDARD_X0_STATE
    X[M, 0] = 1.01
    rng = np.random.default_rng(seed)
    Z = np.tile(nodes, (B, 1, 1))
    Z[:, :, 7:] *= 1.0 + 1e-2 * rng.uniform(-1.0, 1.0, size=(B, M, 7))
    Z = Z.reshape(B, -1)
    if free_tf:
        Z = np.hstack([Z, (tf * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, size=B)))[:, None]])
    return dict(model="goddard", o=o, prob=Problem(7, mode_t, mode_x, time, X), N=N_STEPS, Z=Z, params=o.params()[:8])


def goddard_degenerate():
    """Fixed node times with a zero-length segment 1; row 1 carries a NaN costate in its first node."""
    c = goddard_m3(times=[0.0, 0.03, 0.03, 0.06], free_tf=False, B=3, seed=8)
    c["Z"][1, 9] = np.nan
    return c


def dint():
    """testDoubleIntegrator's problem (M = 1, free tf) around its golden solution: 20 slabs at 9 groups per wave, one idle lane."""
    from oracle.oracle import Oracle, Problem, MODEL_DINT, FIXED, FREE
    z = np.array(json.load(open(os.path.join(GOLD, "dint_flow.json")))["basic_order0_xtol1e-08"][0]["z"])
    o = Oracle(MODEL_DINT, step_nbr=N_STEPS)
    Xi = np.zeros(12)
    Xi[6:] = 0.01
    Xf = np.zeros(12)
    Xf[0], Xf[1] = 10.0, 15.0
    prob = Problem(6, [FIXED, FREE], np.zeros((2, 6), dtype=np.int32), np.array([0.0, 10.0]), np.vstack([Xi, Xf]))
    Z = perturbed(z, 20, 0.05, seed=5)
    Z[3, 12], Z[4, 12] = 2.0, 0.8           # short horizons: dv/dp ~ t^2/2 outweighs dx/dp ~ t^3/6 and the elimination swaps rows
    Z[5, 6:12] *= 30.0                      # a saturated control
    return dict(model="dint", o=o, prob=prob, N=N_STEPS, Z=Z, params=o.params()[:3])


def covid():
    """testCovid19's layout at M = 4 on a trajectory, 7 rows: 28 slabs at 12 groups per wave (d = 4, four idle lanes)."""
    from oracle.oracle import Oracle, Problem, MODEL_COVID, FIXED, FREE, CONTINUOUS
    o = Oracle(MODEL_COVID, step_nbr=N_STEPS)
    o.m.p[0], o.m.p[1], o.m.p[2] = 3.4, 14.0, 5.0
    M = 4
    Xi = np.array([0.93, 0.003, 0.01, 0.057, -0.001, 0.001, 0.0, 0.0])
    time = np.array([30.0 * i / M for i in range(M + 1)])
    X = np.zeros((M + 1, 8))
    X[0], X[M, 3] = Xi, 0.6
    nodes = np.stack([Xi] + [o.traj(0.0, Xi, time[i]) for i in range(1, M)])
    mode_t = [FIXED] + [CONTINUOUS] * (M - 1) + [FIXED]
    mode_x = np.zeros((M + 1, 4), dtype=np.int32)
    mode_x[1:M] = CONTINUOUS
    mode_x[M, :3] = FREE
    return dict(model="covid", o=o, prob=Problem(4, mode_t, mode_x, time, X), N=N_STEPS, Z=perturbed(nodes.ravel(), 7, 0.02, seed=3),
                params=o.params()[:8])


def lqr1d(N=N_STEPS, Z=None, T=None):
    """tests/plugin/lqr1d_plugin.hip.  Default: M = 4 with a free final time, 9 rows: 36 slabs at 21 groups per wave.  With Z and T:
    single shooting over [0, T] from the given rows."""
    from oracle.oracle import Problem, FIXED, FREE, CONTINUOUS
    if Z is not None:
        prob = Problem(2, [FIXED, FIXED], np.zeros((2, 2), dtype=np.int32), np.array([0.0, T]), np.zeros((2, 4)))
        return dict(model="lqr1d", o=None, prob=prob, N=N, Z=np.atleast_2d(Z), params=np.array([1.0]))
    M = 4
    mode_t = [FIXED] + [CONTINUOUS] * (M - 1) + [FREE]
    mode_x = np.zeros((M + 1, 2), dtype=np.int32)
    mode_x[1:M] = CONTINUOUS
    Xn = np.zeros((M + 1, 4))
    Xn[M, 0] = 1.0
    rng = np.random.default_rng(2)
    Z = rng.uniform(-2.0, 2.0, size=(9, 4 * M + 1)) * np.logspace(-1, 2, 9)[:, None]
    Z[:, -1] = np.linspace(0.5, 6.0, 9)
    return dict(model="lqr1d", o=None, prob=Problem(2, mode_t, mode_x, np.linspace(0.0, 1.0, M + 1), Xn), N=N, Z=Z, params=np.array([1.0]))


def osc1d(N=N_STEPS, w=4.0, Z=None, T=4.0):
    """tests/plugin/osc1d_plugin.hip over [0, T]: single shooting; 35 rows = 35 slabs at 32 groups per wave.  The certain sign change."""
    from oracle.oracle import Problem, FIXED
    if Z is None:
        rng = np.random.default_rng(4)
        Z = rng.uniform(0.2, 1.0, size=(35, 2)) * rng.choice([-1.0, 1.0], size=(35, 2))
    prob = Problem(1, [FIXED, FIXED], np.zeros((2, 1), dtype=np.int32), np.array([0.0, T]), np.zeros((2, 2)))
    return dict(model="osc1d", o=None, prob=prob, N=N, Z=np.atleast_2d(Z), params=np.array([w]))


CASES = {"goddard_single": goddard_single, "goddard_m3_free_tf": goddard_m3, "goddard_degenerate": goddard_degenerate, "dint": dint,
         "covid": covid, "lqr1d": lqr1d, "osc1d": osc1d}
_CASE, _REF = {}, {}


def case(name):
    if name not in _CASE:
        c = CASES[name]()
        c["Z"].setflags(write=False)
        _CASE[name] = c
    return _CASE[name]


def timeline(c, prob, z):
    """Node times of a row.  The plugin cases have no oracle: their structures have fixed or uniformly interpolated times only."""
    if c["o"] is not None:
        return np.asarray(c["o"].timeline(prob, z))
    from oracle.oracle import FREE
    M = prob.M
    tf = z[-1] if prob.mode_t[M] == FREE else prob.time[M]
    t0 = prob.time[0]
    return np.array([t0 + k * (tf - t0) / M if 0 < k < M else (t0 if k == 0 else tf) for k in range(M + 1)])


def stepper(c, params):
    if c["model"] == "osc1d":
        return jr.rk4_of(jr.osc1d_rhs(float(params[0])))
    if c["model"] == "lqr1d":
        return jr.rk4_of(jr.lqr1d_rhs(float(params[0])))
    o = c["o"]
    o.set_params(params)
    return lambda t, X, h: o.rk4_step(t, X, h)


def reference_of(c, epsfcn=0.0, stride=7, skip=2, blocks=None, rows=None):
    """slabs[b][i] of tests/jacobi_reference.py for the rows of a case (blocks = (params, time, xnode), any of them None)."""
    from oracle.oracle import Problem
    prob, D = c["prob"], c["prob"].dim
    pp, tt, xx = blocks if blocks is not None else (None, None, None)
    out = []
    for b in (range(len(c["Z"])) if rows is None else rows):
        z = c["Z"][b]
        pb = Problem(D, prob.mode_t, prob.mode_x, prob.time if tt is None else tt[b], prob.xnode if xx is None else xx[b])
        step = stepper(c, c["params"] if pp is None else pp[b][:len(c["params"])])
        tl = timeline(c, pb, z)
        out.append([jr.jacobi_segment(step, D, float(tl[i]), float(tl[i + 1]), z[2 * D * i:2 * D * (i + 1)], c["N"], jr.fd_eps(epsfcn),
                                      stride=stride, skip=skip) for i in range(prob.M)])
    if c["o"] is not None:
        c["o"].set_params(c["params"])
    return out


def reference(name, epsfcn=0.0, stride=7, skip=2):
    key = (name, epsfcn, stride, skip)
    if key not in _REF:
        _REF[key] = reference_of(case(name), epsfcn, stride, skip)
    return _REF[key]
