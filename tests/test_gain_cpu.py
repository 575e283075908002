"""CPU: the definition of socp_gain_batch as tests/gain_reference.py restates it, on the polished nominal Goddard roots of
tests/newton_cases.py (M = 1, N = 50, fixed final time: mu2 = 1 and mu2 = 0.2) and on the double integrator with its final time fixed
at the root's.  Every check is made on 240-bit numbers (mpmath), the step sequence that of the doubles.
(1) chain rule: the gain from the product of blocks against the gain from ONE transition matrix over the tail, at every sample;
(2) meaning: x(t_q) moved by delta e_j with the costate corrected by delta Kp[:, j] misses the terminal rows at second order;
(3) start of the flight: Kp at sample 0 is dz/dx0 of tests/sensitivity_reference.py with SOCP_DIR_XNODE directions;
(4) the instrument: wrong restatements miss the 240-bit gain by a large fraction of its scale;
(5) accuracy of the doubles, a report;  (6) the symbols.  No GPU; the library is only asked for its symbols.

Measured (profiles/gain_cpu_tests.txt): see the lines of the run on record there."""
import os

import numpy as np
import pytest

import exact_jacobian_reference as ej
import fields_reference as fr
import gain_reference as gr
import newton_cases as nc
import sensitivity_reference as sr
import tangent_reference as tr

pytestmark = pytest.mark.skipif(not fr.HAVE_MPMATH, reason="mpmath is the 240-bit carrier")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mpf = fr.mpf
N = nc.N
TOL_CHAIN = mpf(2) ** -200
_CACHE = {}


def record(key, line):
    """The figures of a run (pytest -s): profiles/gain_cpu_tests.txt keeps the lines of the run on record."""
    print("[gain_cpu %s] %s" % (key, line))


def case(name):
    """dict(model, P, sw, D, prob, z, tl, mode_final): a polished root with every time FIXED."""
    def build():
        from oracle.oracle import Problem, FIXED
        if name == "dint":
            c = nc.dint()                                             # free t_f: fixed here at the root's
            p = c["prob"]
            prob = Problem(6, [FIXED, FIXED], p.mode_x, np.array([0.0, float(c["root"][-1])]), p.xnode)
            z = np.array(c["root"][:12])
        else:
            c = nc.goddard(1.0 if name == "goddard" else 0.2)
            prob, z = c["prob"], np.array(c["root"])
        assert all(int(m) == FIXED for m in prob.mode_t) and prob.M == 1
        return dict(model=c["model"], P=[float(v) for v in c["params"]], sw=(0.0, 0.0), D=prob.dim, prob=prob, z=z,
                    tl=[float(t) for t in prob.time], mode_final=prob.mode_x[1])
    return nc.cached(("gain", name), build)


def rows(name, stride, high, mutate=()):
    key = (name, stride, high, tuple(mutate))
    if key not in _CACHE:
        with fr.mpmath.workprec(240):
            c = case(name)
            _CACHE[key] = gr.gain_row(c["model"], c["P"], c["sw"], c["D"], c["tl"], c["mode_final"], c["z"], N, stride, high=high,
                                      mutate=mutate)[0]
    return _CACHE[key]


def big(A):
    return max(abs(mpf(v)) if not isinstance(v, float) else abs(mpf(v)) for v in np.asarray(A, dtype=object).ravel())


def off(A, truth):
    """max |a - truth| / max |truth| in 240 bits."""
    a, t = np.asarray(A, dtype=object).ravel(), np.asarray(truth, dtype=object).ravel()
    return max(abs(mpf(x) - y) for x, y in zip(a, t)) / big(truth)


# ---- (1) the chain rule ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,stride", [("goddard", 7), ("goddard", 10), ("goddard_mu02", 25), ("dint", 7), ("dint", 10)])
def test_1_product_of_blocks_against_one_tail_matrix(name, stride):
    """N = 50: stride 7 does not divide it (seven blocks of 7 steps and one of 1), strides 10 and 25 do."""
    c = case(name)
    with fr.mpmath.workprec(240):
        r = rows(name, stride, True)
        steps, _ = gr.step_sequence(c["tl"][0], c["tl"][1], N)
        assert r["count"] == -(-N // stride) and len(steps) == N
        E = gr.selector(c["mode_final"], c["D"], high=True)
        worst_w, worst_k, solved = mpf(0), mpf(0), 0
        for q in range(r["count"]):
            phi, _ = gr.run_block(c["model"], c["P"], c["sw"], r["xq"][q], steps[q * stride:], high=True)     # a fields-style run from sample q
            W = gr.matmul(E, phi, high=True)
            worst_w = max(worst_w, off(r["wq"][q], W))
            K, info = gr.gain_of(W, c["D"], high=True)
            assert info == r["info"][q], "the same samples are singular"
            if info == 0:
                solved += 1
                worst_k = max(worst_k, off(r["kp"][q], K))
    record("1 %s stride %d" % (name, stride), "%d samples, %d with a gain: product of blocks against one tail matrix, W %.3e, Kp %.3e of their scale "
           "(bar 2^-200 = %.3e)" % (r["count"], solved, float(worst_w), float(worst_k), float(TOL_CHAIN)))
    assert solved >= 1 and r["info"][0] == 0
    assert worst_w <= TOL_CHAIN and worst_k <= TOL_CHAIN


# ---- (2) the meaning ------------------------------------------------------------------------------------------------------------------

def flow_high(c, X, steps):
    """The value state after `steps` from X, in 240 bits (one state, its derivative part zero)."""
    cls, K = fr.DualMpf, fr.DualMpfKit()
    Pn, swn = [mpf(p) for p in c["P"]], [mpf(s) for s in c["sw"]]
    Y = [cls(mpf(x), mpf(0)) for x in X]
    for t, h in steps:
        Y = fr.rk4_dual(fr.RHS[c["model"]], K, cls, Pn, swn, mpf(t), Y, mpf(h), mpf(0))
    return [y.v for y in Y]


def terminal_rows(c, X):
    D = c["D"]
    xd = c["prob"].xnode[1]
    return [X[D + j] if int(c["mode_final"][j]) == gr.FREE else X[j] - mpf(float(xd[j])) for j in range(D)]


@pytest.mark.parametrize("name", ["goddard", "goddard_mu02", "dint"])
def test_2_corrected_miss_is_second_order(name):
    """delta = 1e-9 max(1, |x_j|), then half of it: chosen so that the 240-bit restatement itself shows the orders (a miss of 1e-18 is
    far above the 240-bit rounding and far below the first saturation or switch of the nominal flight)."""
    c, stride = case(name), 7
    D = c["D"]
    with fr.mpmath.workprec(240):
        r = rows(name, stride, True)
        steps, _ = gr.step_sequence(c["tl"][0], c["tl"][1], N)
        lines, ok = [], True
        for q in (0, 2):
            assert r["info"][q] == 0
            tail = steps[q * stride:]
            X = [mpf(v) for v in r["xq"][q]]
            nominal = terminal_rows(c, flow_high(c, X, tail))
            for j in (0, D - 1):
                miss = {}
                for corrected in (True, False):
                    for half in (0, 1):
                        delta = mpf("1e-9") * max(mpf(1), abs(X[j])) / (2 ** half)
                        Y = list(X)
                        Y[j] = Y[j] + delta
                        if corrected:
                            for rr in range(D):
                                Y[D + rr] = Y[D + rr] + delta * r["kp"][q][j][rr]          # column j of K (Kp is column-major)
                        rows_ = terminal_rows(c, flow_high(c, Y, tail))
                        miss[corrected, half] = max(abs(a - b) for a, b in zip(rows_, nominal))
                rc, ru = miss[True, 0] / miss[True, 1], miss[False, 0] / miss[False, 1]
                lines.append("q %d x_%d: corrected %.3e -> %.3e (ratio %.3f), uncorrected %.3e -> %.3e (ratio %.3f)"
                             % (q, j, float(miss[True, 0]), float(miss[True, 1]), float(rc), float(miss[False, 0]), float(miss[False, 1]), float(ru)))
                # a flow that is LINEAR along the flight (the unsaturated double integrator) has no second-order term: its corrected
                # miss is zero to the 240-bit rounding and has no ratio to read -- that is asked for instead, and it asks more
                linear = miss[True, 0] <= TOL_CHAIN * miss[False, 0] and miss[True, 1] <= TOL_CHAIN * miss[False, 1]
                ok = ok and (linear or rc >= 3) and mpf("1.8") <= ru <= mpf("2.2") and miss[True, 0] < miss[False, 0] * mpf("1e-4")
    for line in lines:
        record("2 " + name, line)
    assert ok, "the corrected miss falls by at least 3 per halving (or is zero to rounding), the uncorrected one by about 2"


# ---- (3) the start of the flight --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["goddard", "goddard_mu02", "dint"])
def test_3_sample_0_is_the_xnode_sensitivity(name):
    """dz/dx0 of the shooting problem's root: with the initial state FIXED, rows D .. 2D of direction c are dp0/dx0_c = column c of K(t0).
    The allowance: 8 x (the deviation of this restatement's doubles from its own 240-bit value + that of the sensitivity restatement's
    doubles from ITS 240-bit value), each as a fraction of max |K|.  The two 240-bit values are not the same number to 240 bits: this
    restatement takes the step sequence of the doubles (t and h as the residual rounds them), the sensitivity restatement forms
    (t2 - t1) / N in 240 bits, so the two recurrences differ by a relative 2^-53 in h; they must agree far below the doubles' own errors."""
    c = case(name)
    D, prob = c["D"], c["prob"]
    dirs = [(tr.DIR_XNODE, j) for j in range(D)]
    args = (c["model"], c["P"], c["sw"], prob, c["z"], N)
    with fr.mpmath.workprec(240):
        s = sr.sensitivity_row(*args, dirs)
        assert s["info"] == 0
        sens = np.array([[s["dz"][k][D + r] for r in range(D)] for k in range(D)])               # [c][r]: the layout of Kp
        Jh, _ = ej.exact_jacobian_row(*args, high=True)
        Gh = sr.sensitivity_g(*args, dirs, high=True)
        A = fr.mpmath.matrix(Jh.tolist())
        sens_h = []
        for k in range(D):
            x = fr.mpmath.lu_solve(A, fr.mpmath.matrix([-g for g in Gh[k]]))
            sens_h.append([x[D + r] for r in range(D)])
        kp, kp_h = np.array(rows(name, 7, False)["kp"][0]), rows(name, 7, True)["kp"][0]
        scale = big(kp_h)
        dev_gain = max(abs(mpf(float(a)) - b) for a, b in zip(kp.ravel(), np.asarray(kp_h, dtype=object).ravel())) / scale
        dev_sens = max(abs(mpf(float(a)) - b) for a, b in zip(sens.ravel(), np.asarray(sens_h, dtype=object).ravel())) / scale
        truths = max(abs(a - b) for a, b in zip(np.asarray(kp_h, dtype=object).ravel(), np.asarray(sens_h, dtype=object).ravel())) / scale
        apart = mpf(float(np.abs(kp - sens).max())) / scale
    record("3 " + name, "Kp at sample 0 against dz/dx0 (XNODE directions), of max|K| = %.3e: the doubles apart %.3e; allowance 8 x (%.3e + %.3e); the two "
           "240-bit values apart %.3e" % (float(scale), float(apart), float(dev_gain), float(dev_sens), float(truths)))
    assert truths <= (dev_gain + dev_sens) / 8, "the two definitions are the same numbers up to the rounding of h"
    assert apart <= 8 * (dev_gain + dev_sens)


# ---- (4) the instrument -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mutation", gr.MUTATIONS)
def test_4_wrong_restatements_miss_the_gain(mutation):
    offs = {}
    with fr.mpmath.workprec(240):
        for name in ("goddard", "dint"):
            truth, wrong = rows(name, 7, True), rows(name, 7, False, mutate=(mutation,))
            q = 0 if mutation != "no_reseed" else 0
            if wrong["info"][q] != 0:
                offs[name] = float("inf")
                continue
            offs[name] = float(off(np.array(wrong["kp"][q]), truth["kp"][q]))
    record("4 " + mutation, "wrong restatement %-15s Kp at sample 0 off by %s of its scale" % (mutation, ", ".join("%s %.3e" % kv for kv in offs.items())))
    assert min(offs.values()) > 1e-2, "a wrong restatement is off by a large fraction of the gain's scale"


# ---- (5) accuracy of the doubles: a report ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["goddard", "goddard_mu02", "dint"])
def test_5_doubles_against_240_bits(name):
    with fr.mpmath.workprec(240):
        d, h = rows(name, 7, False), rows(name, 7, True)
        assert d["count"] == h["count"] == 8
        per = []
        for q in range(d["count"]):
            if h["info"][q] == 0 and d["info"][q] == 0:
                per.append("%.2e" % float(off(np.array(d["kp"][q]), h["kp"][q])))
            else:
                per.append("info %d/%d" % (d["info"][q], h["info"][q]))
        wdev = max(float(off(d["wq"][q], h["wq"][q])) for q in range(d["count"]))
    record("5 " + name, "doubles against 240 bits, stride 7: Kp by sample %s; W at most %.2e of its scale" % (" ".join(per), wdev))
    assert d["info"][0] == 0


# ---- (6) the symbols -------------------------------------------------------------------------------------------------------------------------

def test_6_symbols_and_launch_table():
    from socp_amd import capi
    L = capi.lib()
    for sym in ("socp_ctx_has_gain", "socp_gain_batch_dev", "socp_gain_batch", "socp_gain_batch_blocks"):
        assert hasattr(L, sym), sym
    for method in ("gain_batch", "gain_batch_dev", "has_gain"):
        assert hasattr(capi.Context, method), method
    launch = open(os.path.join(ROOT, "socp_amd", "csrc", "launch.hpp")).read()
    assert "kPluginAbi = 18" in launch and "(*gain)" in launch
    assert "kernels_gain.o" in open(os.path.join(ROOT, "socp_amd", "csrc", "Makefile")).read()
