"""CPU: the definition of socp_gain_free_batch as tests/gain_free_reference.py restates it, on polished roots whose final time is FREE:
nominal Goddard (mu2 = 1, M = 1, N = 50: tests/newton_cases.py's root with t_f released and polished again), the double integrator
(nc.dint(), n = 13) and an M = 3 Goddard problem (jacobi_cases.goddard_m3(free_tf=True), N = 10, timeline weights 1/3) polished by
newton_reference.  Every check is made on 240-bit numbers (mpmath).
(1) chain rule: W, wtau and Ke from the product of blocks against ONE tail run from the sample (Psi and l of a single block to the
    end of the sample's segment, then one block per later segment);
(2) meaning: x at the sample moved by delta e_j, p corrected by delta K_p[:, j] and t_f by delta k_t[j], the remaining steps re-timed
    with the step count kept: the d terminal rows AND H miss at second order;
(3) start of the flight: (K_p, k_t) at sample 0 is dz/dx0 of tests/sensitivity_reference.py with SOCP_DIR_XNODE directions -- rows
    D .. 2D and entry n - 1; with M = 3 this is what catches a wrong w_i;
(4) the instrument: wrong restatements miss the 240-bit gain by a stated fraction of its scale;
(5) one block per segment, M = 1: Psi_0 and l_0 are the exact Jacobian's state block and t_f column, bit for bit;
(6) the symbols.  No GPU; the library is only asked for its symbols.

Measured (profiles/gain_free_cpu_tests.txt): see the lines of the run on record there."""
import os

import numpy as np
import pytest

import exact_jacobian_reference as ej
import fields_reference as fr
import gain_free_reference as gf
import gain_reference as gr
import jacobi_cases as jc
import newton_cases as nc
import newton_reference as nr
import sensitivity_reference as sr
import tangent_reference as tr

pytestmark = pytest.mark.skipif(not fr.HAVE_MPMATH, reason="mpmath is the 240-bit carrier")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mpf = fr.mpf
TOL_CHAIN = mpf(2) ** -200
_CACHE = {}
# (4): the fraction of max |Ke| a wrong restatement must miss by at sample 0 -- a factor 10 below the smallest miss measured over the
# cases it is tried on (profiles/gain_free_cpu_tests.txt keeps the measured figures).  Without the l term the border column is zero
# and the system exactly singular (info != 0, counted as an infinite miss) in every case: its bar only asks for that.  w_i = 1 can
# only show where a weight is not 1: M = 3
MUTATION_BARS = {"no_len": 1e300, "w_one": 1.0e-3, "len_after": 7.4e-3, "gradh_unreseeded": 2.0e-4, "border_sign": 3.1e-3, "reseed_time": 7.9e-4}
MUTATION_CASES = {"w_one": ("goddard_m3",)}


def record(key, line):
    """The figures of a run (pytest -s): profiles/gain_free_cpu_tests.txt keeps the lines of the run on record."""
    print("[gain_free_cpu %s] %s" % (key, line))


def case(name):
    """dict(model, P, sw, D, prob, z, N, stride): a polished root whose final time is FREE."""
    def build():
        from oracle.oracle import Problem, FIXED, FREE
        if name == "dint":
            c = nc.dint()
            prob, z, N, stride, r = c["prob"], np.array(c["root"]), nc.N, 7, c["polish"]
        elif name == "goddard":
            c = nc.goddard(1.0)
            p = c["prob"]
            prob = Problem(7, [FIXED, FREE], p.mode_x, p.time, p.xnode)
            z0 = np.concatenate([c["root"], [float(p.time[1])]])
            r = nr.newton_reference("goddard", c["o"], prob, 8, nc.N, z0[None], nc.POLISH)
            z, N, stride = r["z"][0], nc.N, 7
        else:
            c = jc.goddard_m3(free_tf=True, B=1)
            prob, N, stride = c["prob"], 10, 3
            r = nr.newton_reference("goddard", jc.goddard_oracle(N), prob, 8, N, c["Z"][:1], dict(nc.POLISH, rounds=60))
            z = r["z"][0]
        assert int(prob.mode_t[prob.M]) == FREE
        record("root " + name, "polished free-t_f root: ||F||inf = %.3e after %d rounds, t_f = %.14f"
               % (float(r["rnorm"][0]), int(np.ravel(r["rounds_used"])[0]), float(z[-1])))
        assert float(r["rnorm"][0]) < 1e-10, "the polish reached a root"
        return dict(model=c["model"], P=[float(v) for v in c["params"]], sw=(0.0, 0.0), D=prob.dim, prob=prob, z=z, N=N, stride=stride)
    return nc.cached(("gain_free", name), build)


def rows(name, stride, high, mutate=()):
    key = (name, stride, high, tuple(mutate))
    if key not in _CACHE:
        with fr.mpmath.workprec(240):
            c = case(name)
            _CACHE[key] = gf.gain_free_row(c["model"], c["P"], c["sw"], c["prob"], c["z"], c["N"], stride, high=high, mutate=mutate)
    return _CACHE[key]


def big(A):
    return max(abs(mpf(v)) for v in np.asarray(A, dtype=object).ravel())


def off(A, truth):
    """max |a - truth| / max |truth| in 240 bits."""
    a, t = np.asarray(A, dtype=object).ravel(), np.asarray(truth, dtype=object).ravel()
    return max(abs(mpf(x) - y) for x, y in zip(a, t)) / big(truth)


def setting(c):
    """What blocks_segment needs of a row, in 240 bits: (carrier, P, switching times, node times, weights)."""
    lay = ej.Layout(c["prob"])
    C = gf._Carrier(lay.S, True)
    zz = [C.num(v) for v in c["z"]]
    nts, weights, nt = gf.timeline(c["prob"], lay, zz, C.num)
    sws = [nt(node) if node >= 0 else C.num(d) for node, d in zip(lay.sw_node, c["sw"])]
    return C, [C.num(p) for p in c["P"]], sws, nts, weights, zz


# ---- (1) the chain rule ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,stride", [("goddard", 7), ("goddard", 10), ("goddard", 25), ("dint", 7), ("dint", 10), ("dint", 25),
                                         ("goddard_m3", 3)])
def test_1_product_of_blocks_against_one_tail_run(name, stride):
    """N = 50: stride 7 does not divide it, strides 10 and 25 do.  M = 3 (N = 10, stride 3): the tail crosses the later segments."""
    c = case(name)
    D, M, S, N = c["D"], c["prob"].M, 2 * c["D"], c["N"]
    with fr.mpmath.workprec(240):
        r = rows(name, stride, True)
        C, Pn, sws, nts, weights, zz = setting(c)
        later = {i: gf.blocks_segment(c["model"], C, Pn, sws, nts[i], nts[i + 1], zz[S * i:S * (i + 1)], N, N + 1, i == M - 1) for i in range(1, M)}
        worst_w, worst_k, solved, samples = mpf(0), mpf(0), 0, 0
        for i in range(M):
            assert r[i]["count"] == -(-N // stride)
            for q in range(r[i]["count"]):
                tail = gf.blocks_segment(c["model"], C, Pn, sws, nts[i], nts[i + 1], r[i]["xq"][q], N, N + 1, i == M - 1, first_step=q * stride)
                assert tail["count"] == 1
                one = gf.sweep([tail] + [later[k] for k in range(i + 1, M)], weights[i:], c["prob"].mode_x[M], D, high=True)[0]
                samples += 1
                worst_w = max(worst_w, off(r[i]["wq"][q], one["wq"][0]))
                assert one["info"][0] == r[i]["info"][q], "the same samples are singular"
                if one["info"][0] == 0:
                    solved += 1
                    worst_k = max(worst_k, off(r[i]["ke"][q], one["ke"][0]))
    record("1 %s stride %d" % (name, stride), "%d samples, %d with a gain: product of blocks against one tail run, [W | wtau] %.3e, Ke %.3e of their "
           "scale (bar 2^-200 = %.3e); info by sample %s" % (samples, solved, float(worst_w), float(worst_k), float(TOL_CHAIN),
                                                             [list(s["info"]) for s in r]))
    assert solved >= 1 and r[0]["info"][0] == 0
    assert worst_w <= TOL_CHAIN and worst_k <= TOL_CHAIN


# ---- (2) the meaning ------------------------------------------------------------------------------------------------------------------

def fly(c, C, Pn, sws, t1, t2, X, N, first_step):
    """The value state at t2 from X at step `first_step` of the segment's loop re-timed over [t1, t2], step count kept; 240 bits."""
    fn, zero = fr.RHS[c["model"]], mpf(0)
    cls, K = fr.DualMpf, fr.DualMpfKit()
    Y = [cls(x, zero) for x in X]
    dt = (t2 - t1) / N
    t = t1
    for _ in range(first_step):
        t = t + dt
    for _ in range(first_step, N):
        h = (t2 - t) if (t + dt > t2) else dt
        Y = fr.rk4_dual(fn, K, cls, Pn, sws, t, Y, h, zero)
        t = t + dt
    return [y.v for y in Y]


def terminal_miss(c, C, Pn, sws, nts, zz, i, k, X, tf):
    """The d terminal rows and H at the end of the flight from X at step k of segment i, the timeline re-timed with t_f = tf."""
    lay = ej.Layout(c["prob"])
    D, S, M, N = c["D"], 2 * c["D"], c["prob"].M, c["N"]
    z2 = list(zz)
    z2[-1] = tf
    nts2, _, _ = gf.timeline(c["prob"], lay, z2, C.num)
    X = fly(c, C, Pn, sws, nts2[i], nts2[i + 1], X, N, k)
    for s in range(i + 1, M):                                         # interior nodes are CONTINUOUS: the flight goes on from its own state
        X = fly(c, C, Pn, sws, nts2[s], nts2[s + 1], X, N, 0)
    xd = c["prob"].xnode[M]
    rows_ = [X[D + j] if int(c["prob"].mode_x[M][j]) == gf.FREE else X[j] - mpf(float(xd[j])) for j in range(D)]
    H = ej.hamiltonian_on(c["model"], fr.DualMpfKit(), Pn, sws, nts2[M], [fr.DualMpf(x, mpf(0)) for x in X])
    return rows_ + [H.v]


@pytest.mark.parametrize("name", ["goddard", "dint", "goddard_m3"])
def test_2_corrected_miss_is_second_order(name):
    """delta = 1e-9 max(1, |x_j|), then half of it, at samples 0 and 2 (for M = 3: sample 0 of segment 0 and sample 2 of segment 1).  The
    bars are test_gain_cpu.py::test_2's: the corrected miss falls by >= 3 per halving (or is zero to 240-bit rounding), the
    uncorrected one by 1.8 .. 2.2, and the corrected one is below 1e-4 of the uncorrected."""
    c = case(name)
    D, M = c["D"], c["prob"].M
    with fr.mpmath.workprec(240):
        r = rows(name, c["stride"], True)
        C, Pn, sws, nts, weights, zz = setting(c)
        lines, ok = [], True
        for i, q in ((0, 0), (M // 2, 2)):
            assert r[i]["info"][q] == 0
            k = q * c["stride"]
            X = [mpf(v) for v in r[i]["xq"][q]]
            nominal = terminal_miss(c, C, Pn, sws, nts, zz, i, k, X, zz[-1])
            for j in (0, D - 1):
                miss = {}
                for corrected in (True, False):
                    for half in (0, 1):
                        delta = mpf("1e-9") * max(mpf(1), abs(X[j])) / (2 ** half)
                        Y = list(X)
                        Y[j] = Y[j] + delta
                        tf = zz[-1]
                        if corrected:
                            for rr in range(D):
                                Y[D + rr] = Y[D + rr] + delta * r[i]["ke"][q][j][rr]
                            tf = tf + delta * r[i]["ke"][q][j][D]
                        got = terminal_miss(c, C, Pn, sws, nts, zz, i, k, Y, tf)
                        miss[corrected, half] = max(abs(a - b) for a, b in zip(got, nominal))
                rc, ru = miss[True, 0] / miss[True, 1], miss[False, 0] / miss[False, 1]
                lines.append("segment %d q %d x_%d: corrected %.3e -> %.3e (ratio %.3f), uncorrected %.3e -> %.3e (ratio %.3f)"
                             % (i, q, j, float(miss[True, 0]), float(miss[True, 1]), float(rc), float(miss[False, 0]), float(miss[False, 1]), float(ru)))
                linear = miss[True, 0] <= TOL_CHAIN * miss[False, 0] and miss[True, 1] <= TOL_CHAIN * miss[False, 1]
                ok = ok and (linear or rc >= 3) and mpf("1.8") <= ru <= mpf("2.2") and miss[True, 0] < miss[False, 0] * mpf("1e-4")
    for line in lines:
        record("2 " + name, line)
    assert ok, "the corrected miss of the terminal rows and of H falls by at least 3 per halving, the uncorrected one by about 2"


# ---- (3) the start of the flight --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["goddard", "dint", "goddard_m3"])
def test_3_sample_0_is_the_xnode_sensitivity(name):
    """dz/dx0 of the shooting problem's root: with the initial state FIXED, rows D .. 2D of direction c are dp0/dx0_c and entry n - 1 is
    dt_f/dx0_c = column c of Ke at sample 0.  The allowance is test_gain_cpu.py::test_3's: 8 x (the deviation of this restatement's doubles
    from its own 240-bit value + that of the sensitivity restatement's doubles from ITS 240-bit value), each as a fraction of max |Ke|."""
    c = case(name)
    D, prob, n = c["D"], c["prob"], len(c["z"])
    dirs = [(tr.DIR_XNODE, j) for j in range(D)]
    args = (c["model"], c["P"], c["sw"], prob, c["z"], c["N"])
    pick = list(range(D, 2 * D)) + [n - 1]
    with fr.mpmath.workprec(240):
        s = sr.sensitivity_row(*args, dirs)
        assert s["info"] == 0
        sens = np.array([[s["dz"][k][e] for e in pick] for k in range(D)])                        # [c][r]: the layout of Ke
        Jh, _ = ej.exact_jacobian_row(*args, high=True)
        Gh = sr.sensitivity_g(*args, dirs, high=True)
        A = fr.mpmath.matrix(Jh.tolist())
        sens_h = []
        for k in range(D):
            x = fr.mpmath.lu_solve(A, fr.mpmath.matrix([-g for g in Gh[k]]))
            sens_h.append([x[e] for e in pick])
        ke, ke_h = np.array(rows(name, c["stride"], False)[0]["ke"][0]), rows(name, c["stride"], True)[0]["ke"][0]
        scale = big(ke_h)
        flat = lambda a: np.asarray(a, dtype=object).ravel()                                       # noqa: E731
        dev_gain = max(abs(mpf(float(a)) - b) for a, b in zip(ke.ravel(), flat(ke_h))) / scale
        dev_sens = max(abs(mpf(float(a)) - b) for a, b in zip(sens.ravel(), flat(sens_h))) / scale
        truths = max(abs(a - b) for a, b in zip(flat(ke_h), flat(sens_h))) / scale
        apart = mpf(float(np.abs(ke - sens).max())) / scale
    record("3 " + name, "Ke at sample 0 against dz/dx0 (XNODE directions: rows D..2D and entry n-1), of max|Ke| = %.3e: the doubles apart %.3e; "
           "allowance 8 x (%.3e + %.3e); the two 240-bit values apart %.3e" % (float(scale), float(apart), float(dev_gain), float(dev_sens), float(truths)))
    assert truths <= (dev_gain + dev_sens) / 8, "the two definitions are the same numbers"
    assert apart <= 8 * (dev_gain + dev_sens)


# ---- (4) the instrument -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mutation", gf.MUTATIONS)
def test_4_wrong_restatements_miss_the_gain(mutation):
    offs = {}
    with fr.mpmath.workprec(240):
        for name in MUTATION_CASES.get(mutation, ("goddard", "dint", "goddard_m3")):
            stride = case(name)["stride"]
            truth, wrong = rows(name, stride, True)[0], rows(name, stride, False, mutate=(mutation,))[0]
            assert truth["info"][0] == 0
            offs[name] = float("inf") if wrong["info"][0] != 0 else float(off(np.array(wrong["ke"][0]), truth["ke"][0]))
    record("4 " + mutation, "wrong restatement %-17s Ke at sample 0 off by %s of its scale (bar %.0e)"
           % (mutation, ", ".join("%s %.3e" % kv for kv in offs.items()), MUTATION_BARS[mutation]))
    assert min(offs.values()) > MUTATION_BARS[mutation], "a wrong restatement is off by a stated fraction of the gain's scale"


def test_4_the_right_restatement_passes_the_same_measure():
    """The doubles of the unmutated restatement sit far below every bar: the instrument separates."""
    with fr.mpmath.workprec(240):
        worst = max(float(off(np.array(rows(name, case(name)["stride"], False)[0]["ke"][0]), rows(name, case(name)["stride"], True)[0]["ke"][0]))
                    for name in ("goddard", "dint", "goddard_m3"))
    record("4 none", "the unmutated doubles: Ke at sample 0 off by at most %.3e of its scale" % worst)
    assert worst < 1e-3 * min(MUTATION_BARS.values())


# ---- (5) one block per segment ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["goddard", "dint"])
def test_5_one_block_is_the_exact_jacobian(name):
    """stride >= the number of steps, M = 1, doubles: the final rows D .. 2D-1 of the exact Jacobian are E Psi_0 (state block) and E l_0
    (t_f column, weight 1.0) -- the selector only picks rows, so the comparison is bit for bit."""
    c = case(name)
    D, S, n = c["D"], 2 * c["D"], len(c["z"])
    r = gf.gain_free_row(c["model"], c["P"], c["sw"], c["prob"], c["z"], c["N"], c["N"] + 3)[0]
    J, _ = ej.exact_jacobian_row(c["model"], c["P"], c["sw"], c["prob"], c["z"], c["N"])
    assert r["count"] == 1
    pick = [D + j if int(c["prob"].mode_x[1][j]) == gf.FREE else j for j in range(D)]
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)                      # noqa: E731
    assert np.array_equal(bits(r["psi"][0][pick, :]), bits(J[D:2 * D, :S])), "Psi_0 rows against the state block"
    assert np.array_equal(bits(r["len"][0][pick]), bits(J[D:2 * D, n - 1])), "l_0 rows against the t_f column"
    assert np.abs(r["len"][0]).max() > 0
    record("5 " + name, "one block: %d rows of Psi_0 and l_0 equal the exact Jacobian's final rows bit for bit; max|l_0| = %.6e" % (D, np.abs(r["len"][0]).max()))


# ---- (6) the symbols -------------------------------------------------------------------------------------------------------------------------

def test_6_symbols_and_launch_table():
    from socp_amd import capi
    L = capi.lib()
    for sym in ("socp_ctx_has_gain_free", "socp_gain_free_batch_dev", "socp_gain_free_batch", "socp_gain_free_batch_blocks"):
        assert hasattr(L, sym), sym
    for method in ("gain_free_batch", "gain_free_batch_dev", "has_gain_free"):
        assert hasattr(capi.Context, method), method
    launch = open(os.path.join(ROOT, "socp_amd", "csrc", "launch.hpp")).read()
    assert "kPluginAbi = 19;" in launch and "(*gain_free)" in launch
    assert "kernels_gain_free.o" in open(os.path.join(ROOT, "socp_amd", "csrc", "Makefile")).read()
