"""The inputs of the Newton-polish tests (helper of test_newton_cpu.py / test_gpu_newton_batch.py, not a test).  Every case is built
from the CPU oracle and tests/newton_reference.py alone, so what the GPU tests rest on -- which row ends in which status, after how
many rounds -- is a property of the restatement's own output and is asserted without a GPU (test_newton_cpu.py).  A case and its
reference are computed once and shared read-only."""
import numpy as np

import jacobi_cases as jc
import newton_reference as nr
from conftest import GODDARD_X0_STATE, GODDARD_PSTAR, goddard_single_problem

N = 50
# the costates of the single-shooting root at mu2 = 0.2, N = 50, to the digits a multiple-shooting homotopy in mu2 (M = 5, steps of
# 0.01 below 0.4) left; single shooting does not survive a step of 0.1 in mu2 (||F||inf = 9.8e+2 after the first)
GODDARD_P_MU02 = np.array([-6.2824366040610649, 4.4407688580054335e-03, 4.4407685217157972e-01, -2.9124176372763344e-01,
                           3.3971421811580067e-04, 3.3971400786990354e-02, 6.1490215675051245e-02])
POLISH = dict(jac=2, ftol=1e-300, rounds=30, trials=8)       # to rounding level: the row ends STALLED
_CACHE = {}


def cached(key, build):
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


def perturbed(z, rel, seed):
    return np.asarray(z) * (1.0 + rel * np.random.default_rng(seed).uniform(-1.0, 1.0, np.shape(z)))


def goddard(mu2=1.0):
    """Nominal Goddard, single shooting (M = 1, n = 14), N = 50, with its root polished by the restatement (jac = 2)."""
    def build():
        o = jc.goddard_oracle(N)
        o.set_param("mu2", mu2)
        prob, _ = goddard_single_problem()
        z0 = np.concatenate([GODDARD_X0_STATE, GODDARD_PSTAR if mu2 == 1.0 else GODDARD_P_MU02])
        r = nr.newton_reference("goddard", o, prob, 8, N, z0[None], POLISH)
        return dict(model="goddard", o=o, prob=prob, N=N, nparams=8, params=o.params()[:8], root=r["z"][0], floor=float(r["rnorm"][0]),
                    polish=r)
    return cached(("goddard", mu2), build)


def dint():
    """testDoubleIntegrator's problem (M = 1, free tf, n = 13) at N = 50, root polished by the restatement (jac = 2)."""
    def build():
        from oracle.oracle import Oracle, MODEL_DINT
        c = jc.dint()
        o = Oracle(MODEL_DINT, step_nbr=N)
        r = nr.newton_reference("dint", o, c["prob"], 3, N, c["Z"][:1], POLISH)
        return dict(model="dint", o=o, prob=c["prob"], N=N, nparams=3, params=o.params()[:3], root=r["z"][0], floor=float(r["rnorm"][0]),
                    polish=r)
    return cached("dint", build)


# ---- the mixed batch of the GPU tests: Goddard M = 1, jac = 2, every status in one call ------------------------------------------
MIXED = dict(jac=2, ftol=1e-12, xtol=1e-8, trials=4, rounds=3)
MIXED_ROWS = 70


def mixed():
    """70 rows drawn from a few distinct ones (a row's result depends on the row alone, so the restatement computes each once), each
    with its own node times: the row whose t_f equals its t_0 has three exactly zero Jacobian columns (SINGULAR)."""
    def build():
        c = goddard(1.0)
        root, prob = c["root"], c["prob"]
        kinds = [("root", root), ("near", perturbed(root, 1e-8, 1)), ("near2", perturbed(root, 1e-7, 1)), ("mid", perturbed(root, 1e-6, 2)),
                 ("mid2", perturbed(root, 1e-6, 3)), ("far", perturbed(root, 1e-3, 4)), ("nan", np.where(np.arange(14) == 9, np.nan, root)),
                 ("flat", root)]
        order = np.random.default_rng(70).integers(0, len(kinds) - 3, MIXED_ROWS)
        order[[3, 40, 69]] = [len(kinds) - 3, len(kinds) - 2, len(kinds) - 1]      # far, nan, flat: once each
        order[[0, 64]] = [3, 4]
        Z = np.stack([kinds[k][1] for k in order])
        time = np.tile(prob.time, (MIXED_ROWS, 1))
        time[69, 1] = time[69, 0]
        ref = nr.newton_reference("goddard", c["o"], prob, 8, N, Z, MIXED, time=time)
        return dict(c, Z=Z, time=time, names=[kinds[k][0] for k in order], ref=ref)
    return cached("mixed", build)
