"""The inputs of the event tests and their CPU references (helper of test_events_cpu.py / test_gpu_events_batch.py, not a test).

Every case is built from the CPU oracle and the golden solutions alone, so that test_events_cpu.py can check, without a GPU, the
condition the GPU tests rest on: at every step end of every row |channel - level| is far above rounding level, hence no
arithmetic flavour can flip a sign and the event SETS of the flavours must agree exactly.  A case's reference (the event lists of
tests/events_reference.py) is computed once per refinement count and shared read-only."""
import json
import os

import numpy as np

from conftest import goddard_c1_problem
from events_reference import reference_events_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def perturbed(z, B, rel, seed):
    """Row 0 = z, rows 1 .. B-1 = z (1 + rel xi), xi uniform(-1, 1) per entry."""
    rng = np.random.default_rng(seed)
    Z = np.tile(np.asarray(z, dtype=np.float64), (B, 1))
    Z[1:] *= 1.0 + rel * rng.uniform(-1.0, 1.0, size=(B - 1, Z.shape[1]))
    return Z


def goddard_stage3_row():
    """The golden stage-3 solution of the testGoddard flow: mu2 continuation, KD = 310, mu2 = 0.2, M = 6, free tf."""
    g = json.load(open(os.path.join(GOLD, "goddard_flow.json")))["goddard_N10_M6"][2]
    assert g["stage"] == "mu2_continuation" and g["info"] == 1 and len(g["z"]) == 85
    return np.array(g["z"])


def goddard_oracle(N, mu2=0.2):
    from oracle.oracle import Oracle, MODEL_GODDARD
    o = Oracle(MODEL_GODDARD, step_nbr=N)
    o.set_param("mu2", mu2)
    return o


def goddard_levels(params):
    """(-2 mu2 u_max, 0): below the first the thrust is saturated, below the second it is on (goddard.cpp:137-176)."""
    return [-2.0 * params[6] * params[4], 0.0]


def _goddard(B, N, seed):
    o = goddard_oracle(N)
    prob, _ = goddard_c1_problem(o)
    Z = perturbed(goddard_stage3_row(), B, 1e-3, seed)
    p = o.params()[:8]
    return dict(model="goddard", o=o, prob=prob, N=N, Z=Z, params=p, chan=[0, 0], levels=np.tile(goddard_levels(p), (B, 1)), blocks=None)


def goddard_b130():
    """780 lanes: twelve full waves and a partial one."""
    return _goddard(130, 10, seed=1)


def goddard_n100():
    return _goddard(8, 100, seed=2)


def goddard_blocks():
    """Every row with its own mu2 (0.15 .. 0.25), hence its own saturation level, its own initial time and node table."""
    c = _goddard(130, 10, seed=3)
    B, prob = 130, c["prob"]
    params = np.tile(np.concatenate([c["params"], [0.0, 0.0]]), (B, 1))
    params[:, 6] = np.linspace(0.15, 0.25, B)
    time = np.tile(prob.time, (B, 1))
    time[:, 0] = 1e-4 * np.sin(np.arange(B))                 # the FIXED initial time is the entry the timeline reads
    xnode = np.tile(prob.xnode.ravel(), (B, 1)) * (1.0 + 1e-3 * np.arange(B))[:, None]
    c["levels"] = np.array([goddard_levels(p) for p in params])
    c["blocks"] = (params, time, xnode)
    return c


def goddard_degenerate():
    """Four segments from the first four node states of the golden row; segment 1 has zero length, segment 2 runs backward."""
    from oracle.oracle import Problem, FIXED, CONTINUOUS
    o = goddard_oracle(10)
    full, _ = goddard_c1_problem(o)
    z = goddard_stage3_row()
    tf = z[84]
    mode_t = [FIXED] * 5
    mode_x = np.zeros((5, 7), dtype=np.int32)
    mode_x[1:4] = CONTINUOUS
    t = np.array([0.0, tf / 6, tf / 6, tf / 8, tf / 3])
    prob = Problem(7, mode_t, mode_x, t, full.xnode[:5])
    Z = perturbed(z[:56], 3, 1e-3, seed=4)
    p = o.params()[:8]
    return dict(model="goddard", o=o, prob=prob, N=10, Z=Z, params=p, chan=[0, 0], levels=np.tile(goddard_levels(p), (3, 1)), blocks=None)


def _midpoint_levels(c):
    """Per row and watch: the midpoint of the oracle's own minimum and maximum of the channel along the row, so that a crossing
    exists by construction."""
    B, E = len(c["Z"]), len(c["chan"])
    lv = np.empty((B, E))
    for b in range(B):
        seen = {}
        reference_events_batch(c["o"], c["prob"], c["Z"][b:b + 1], c["N"], c["chan"], np.zeros((1, E)), 0, channels=seen)
        for e, ch in enumerate(c["chan"]):
            lv[b, e] = 0.5 * (min(seen[ch]) + max(seen[ch]))
    return lv


def dint_basic():
    """testDoubleIntegrator's problem (M = 1, free tf) at its golden solution and two perturbed copies; |u| against the midpoint."""
    from oracle.oracle import Oracle, Problem, MODEL_DINT, FIXED, FREE
    z = np.array(json.load(open(os.path.join(GOLD, "dint_flow.json")))["basic_order0_xtol1e-08"][0]["z"])
    assert len(z) == 13
    N = 30
    o = Oracle(MODEL_DINT, step_nbr=N)
    Xi = np.zeros(12)
    Xi[6:] = 0.01
    Xf = np.zeros(12)
    Xf[0], Xf[1] = 10.0, 15.0
    prob = Problem(6, [FIXED, FREE], np.zeros((2, 6), dtype=np.int32), np.array([0.0, 10.0]), np.vstack([Xi, Xf]))
    c = dict(model="dint", o=o, prob=prob, N=N, Z=perturbed(z, 3, 1e-3, seed=5), params=o.params()[:3], chan=[0], blocks=None)
    c["levels"] = _midpoint_levels(c)
    return c


def covid_m20():
    """testCovid19's problem (M = 20, tf = 30 days) at its golden solution and a perturbed copy, 50 steps per segment; both
    channels against their midpoints."""
    from oracle.oracle import Oracle, Problem, MODEL_COVID, FIXED, FREE, CONTINUOUS
    z = np.array(json.load(open(os.path.join(GOLD, "covid_flow.json")))[0]["z"])
    assert len(z) == 160
    N, M = 50, 20
    o = Oracle(MODEL_COVID, step_nbr=N)
    o.m.p[0], o.m.p[1], o.m.p[2] = 3.4, 14.0, 5.0            # R0, Tinf, Tinc (testCovid19.cpp:41-43)
    mode_t = [FIXED] + [CONTINUOUS] * (M - 1) + [FIXED]
    mode_x = np.full((M + 1, 4), CONTINUOUS, dtype=np.int32)
    mode_x[0] = FIXED
    mode_x[M] = [FREE, FREE, FREE, FIXED]
    X = np.zeros((M + 1, 8))
    X[0] = [0.93, 0.003, 0.01, 0.057, -0.001, 0.001, 0.0, 0.0]
    X[M, 3] = 0.6
    prob = Problem(4, mode_t, mode_x, np.array([30.0 * i / M for i in range(M + 1)]), X)
    c = dict(model="covid", o=o, prob=prob, N=N, Z=perturbed(z, 2, 1e-3, seed=6), params=o.params()[:8], chan=[0, 1], blocks=None)
    c["levels"] = _midpoint_levels(c)
    return c


CASES = {"goddard_b130": goddard_b130, "goddard_n100": goddard_n100, "goddard_blocks": goddard_blocks,
         "goddard_degenerate": goddard_degenerate, "dint_basic": dint_basic, "covid_m20": covid_m20}
_CASE, _REF, _MARGIN = {}, {}, {}


def case(name):
    if name not in _CASE:
        c = CASES[name]()
        for key in ("Z", "levels"):
            c[key].setflags(write=False)
        _CASE[name] = c
    return _CASE[name]


def reference(name, R):
    """The event lists [b][i] of a case at R refinement steps; the first call of a case also records its margin."""
    if (name, R) not in _REF:
        c = case(name)
        blocks = c["blocks"] or (None, None, None)
        margins = []
        _REF[name, R] = reference_events_batch(c["o"], c["prob"], c["Z"], c["N"], c["chan"], c["levels"], R, params=blocks[0], time=blocks[1],
                                               xnode=blocks[2], margins=margins)
        _MARGIN.setdefault(name, min(margins) if margins else np.inf)
    return _REF[name, R]


def margin(name):
    """min |channel - level| over all watches, step ends and rows of a case."""
    reference(name, 0)
    return _MARGIN[name]
