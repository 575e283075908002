"""The inputs of the exact-sensitivity tests (helper of test_sensitivity_cpu.py / test_gpu_sensitivity_batch.py, not a test).  Every
case is built from the CPU oracle and the restatements alone.  A case carries its directions: every kind, the entries the modes never
read included.  A case and its reference are computed once and shared read-only."""
import numpy as np

import jacobi_cases as jc
from conftest import goddard_single_problem
from tangent_reference import DIR_PARAM, DIR_TIME, DIR_XNODE

_CACHE = {}


def cached(key, build):
    if key not in _CACHE:
        _CACHE[key] = build()
        for v in _CACHE[key].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _CACHE[key]


def params_of(indices):
    return [(DIR_PARAM, q) for q in indices]


def goddard_single(N=10):
    """Nominal Goddard, single shooting (M = 1, n = 14), smooth law; 5 rows around the extremal.  16 directions: the eight parameters,
    both node times (FIXED), five boundary values that are read and one that is not (component 3 of node 1 is FREE)."""
    def build():
        o = jc.goddard_oracle(N)
        prob, z = goddard_single_problem()
        dirs = params_of(range(8)) + [(DIR_TIME, 0), (DIR_TIME, 1)] + [(DIR_XNODE, c) for c in (0, 3, 6)] + [(DIR_XNODE, 14 + c) for c in (0, 2, 3)]
        return dict(model="goddard", prob=prob, N=N, Z=jc.perturbed(z, 5, 1e-3, seed=11), params=o.params()[:8], sw=(0.0, 0.0), nparams=8,
                    dirs=dirs, unread=[15])
    return cached(("goddard_single", N), build)


def goddard_m3(N=4, general=False):
    """Goddard, M = 3 with a FREE tf (n = 43, the interior nodes interpolated and CONTINUOUS); 3 rows.  general: mu2 = 0 -- full thrust up
    to sw0 = 0.02, the closed-form singular control up to sw1 = 0.05, then off -- with only the parameters the definition differentiates
    there (mu2 sits on the law's own threshold and u_max on the saturation's).  The table time of a CONTINUOUS or FREE node is not read."""
    def build():
        c = jc.goddard_m3(B=3, seed=9)
        P = np.array(c["params"], dtype=np.float64)
        if general:
            P[6] = 0.0
        dirs = params_of((0, 1, 2, 3, 5, 7) if general else range(8)) + [(DIR_TIME, j) for j in range(4)]
        dirs += [(DIR_XNODE, 0), (DIR_XNODE, 14), (DIR_XNODE, 42), (DIR_XNODE, 45)]
        return dict(model="goddard", prob=c["prob"], N=N, Z=np.array(c["Z"]), params=P, sw=(0.02, 0.05) if general else (0.0, 0.0), nparams=8,
                    dirs=dirs, unread=[len(dirs) - 7, len(dirs) - 6, len(dirs) - 5, len(dirs) - 3, len(dirs) - 1])
    return cached(("goddard_m3", N, general), build)


def dint_fixed_node_free_tf(N=6):
    """The double integrator, M = 2 with a FIXED interior node (both sides pinned to xd, its time read from the table) and a FREE tf;
    segment 1 saturates the control; 3 rows."""
    def build():
        from oracle.oracle import Oracle, Problem, MODEL_DINT, FIXED, FREE
        o = Oracle(MODEL_DINT, step_nbr=N)
        n0 = np.array([0.0, 0.0, 0.0, 0.3, -0.2, 0.1, 0.02, -0.01, 0.015, 0.4, -0.3, 0.2])
        n1 = np.array([0.5, -0.3, 0.2, 0.1, 0.1, -0.2, 0.02, -0.01, 0.015, 2.0, -1.5, 1.0])
        Z = np.tile(np.concatenate([n0, n1, [3.0]]), (3, 1)) * (1.0 + 0.05 * np.random.default_rng(3).uniform(-1.0, 1.0, size=(3, 25)))
        mode_x = np.zeros((3, 6), dtype=np.int32)
        mode_x[2, 3:] = FREE
        X = np.zeros((3, 12))
        X[1, :6] = [0.45, -0.25, 0.2, 0.1, 0.1, -0.2]
        X[2, :3] = [1.0, -0.5, 0.3]
        prob = Problem(6, [FIXED, FIXED, FREE], mode_x, np.array([0.0, 1.5, 3.0]), X)
        dirs = params_of(range(3)) + [(DIR_TIME, 0), (DIR_TIME, 1), (DIR_TIME, 2)]
        dirs += [(DIR_XNODE, 1), (DIR_XNODE, 12), (DIR_XNODE, 17), (DIR_XNODE, 24), (DIR_XNODE, 28)]
        return dict(model="dint", prob=prob, N=N, Z=Z, params=o.params()[:3], sw=(0.0, 0.0), nparams=3, dirs=dirs, unread=[5, 10])
    return cached(("dint", N), build)


def covid_m2(N=6):
    """covid19, M = 2, fixed times, CONTINUOUS interior node; node 0 with the control on its upper bound -- the control IS umax there --
    node 1 with I >= Imax (the penalty); 3 rows."""
    def build():
        from oracle.oracle import Oracle, Problem, MODEL_COVID, FIXED, CONTINUOUS
        o = Oracle(MODEL_COVID, step_nbr=N)
        n0 = np.array([0.9, 0.01, 0.05, 0.04, -1500.0, 300.0, 0.5, 0.1])
        n1 = np.array([0.6, 0.05, 0.2, 0.15, -0.5, 0.8, 0.3, 0.1])
        Z = np.tile(np.concatenate([n0, n1]), (3, 1)) * (1.0 + 0.02 * np.random.default_rng(4).uniform(-1.0, 1.0, size=(3, 16)))
        mode_x = np.zeros((3, 4), dtype=np.int32)
        mode_x[1] = CONTINUOUS
        prob = Problem(4, [FIXED, FIXED, FIXED], mode_x, np.array([0.0, 5.0, 10.0]), np.zeros((3, 8)))
        dirs = params_of(range(8)) + [(DIR_TIME, 0), (DIR_TIME, 1), (DIR_TIME, 2), (DIR_XNODE, 2), (DIR_XNODE, 9), (DIR_XNODE, 19)]
        return dict(model="covid", prob=prob, N=N, Z=Z, params=o.params()[:8], sw=(0.0, 0.0), nparams=8, dirs=dirs, unread=[12])
    return cached(("covid", N), build)


def osc1d_plugin(N=10):
    """tests/plugin/osc1d_sensitivity_plugin.hip, M = 2 with a FREE interior time and a FREE tf: its switching row reads X+ and the
    parameter on both sides; 5 rows."""
    def build():
        from oracle.oracle import Problem, FIXED, FREE, CONTINUOUS
        rng = np.random.default_rng(5)
        Z = np.hstack([rng.uniform(0.2, 1.0, size=(5, 4)), rng.uniform(0.8, 1.2, size=(5, 1)), rng.uniform(2.0, 2.5, size=(5, 1))])
        mode_x = np.zeros((3, 1), dtype=np.int32)
        mode_x[1] = CONTINUOUS
        prob = Problem(1, [FIXED, FREE, FREE], mode_x, np.array([0.0, 1.0, 2.0]), np.zeros((3, 2)))
        dirs = [(DIR_PARAM, 0), (DIR_TIME, 0), (DIR_TIME, 1), (DIR_XNODE, 0), (DIR_XNODE, 4)]
        return dict(model="osc1d", prob=prob, N=N, Z=Z, params=np.array([4.0]), sw=(0.0, 0.0), nparams=1, dirs=dirs, unread=[2])
    return cached(("osc1d", N), build)


CASES = {"goddard_single": goddard_single, "goddard_m3": goddard_m3, "goddard_m3_general": lambda: goddard_m3(general=True),
         "dint_fixed_node_free_tf": dint_fixed_node_free_tf, "covid_m2": covid_m2, "osc1d_plugin": osc1d_plugin}
