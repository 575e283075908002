"""CPU: the definition of socp_extrema_batch as tests/extrema_reference.py restates it -- (1) the surface exists; (2) on rows built
with the CPU oracle the sequential reduction equals the argmin / argmax brute force; (3) the conventions the strict comparisons give;
(4) the instrument: three wrong restatements differ from it on those rows; (5) the figure the feature is for, the spread of the
Hamiltonian along the nominal Goddard extremal at three step numbers.  No GPU; the library is only asked for its symbols.

Measured (profiles/extrema_cpu_tests.txt): the spread of H over the rows of the nominal Goddard start (mu2 = 1, [0, 0.2640825]) is
1.644e+01 at N = 10 (ten steps do not resolve this start: H leaves 6e-3 for -16 in the last step), 1.176e-05 at N = 100 and
1.840e-08 at N = 1000 (H = 8.576e-06 at t = 0): between the last two it falls by 640, short of the 10^4 of a fourth-order method."""
import os
import subprocess
import sys

import numpy as np
import pytest

import extrema_reference as er
from conftest import GODDARD_X0_STATE, GODDARD_PSTAR, GODDARD_TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("socp_extrema_width", "socp_ctx_has_extrema", "socp_extrema_batch_dev", "socp_extrema_batch", "socp_extrema_batch_blocks")


def test_library_header_python_layer_and_sweep_tool_have_the_feature():
    """Fails without the feature."""
    from socp_amd import capi
    from test_capi_symbols import declared_functions
    declared = declared_functions()
    L = capi.lib()
    for name in SYMBOLS:
        assert name in declared, name + " is not declared in include/"
        assert hasattr(L, name), name + " is not exported"
    header = open(os.path.join(ROOT, "include", "socp_hip.h")).read()
    for macro, value in (("SOCP_EXTREMA_CONTROL", 1), ("SOCP_EXTREMA_HAMILTONIAN", 2), ("SOCP_EXTREMA_EVENTS", 4)):
        assert any(ln.split()[:3] == ["#define", macro, str(value)] for ln in header.splitlines()), macro
    assert (capi.EXTREMA_CONTROL, capi.EXTREMA_HAMILTONIAN, capi.EXTREMA_EVENTS) == (1, 2, 4)
    assert len(L.socp_extrema_batch_dev.argtypes) == 10
    assert len(L.socp_extrema_batch.argtypes) == 10 and len(L.socp_extrema_batch_blocks.argtypes) == 14
    for name in ("has_extrema", "extrema_width", "extrema_batch_dev", "extrema_batch", "extrema_channels"):
        assert callable(getattr(capi.Context, name)), name
    assert capi.extrema_channel_names(2, 1, 2) == ["x0", "x1", "p0", "p1", "u0", "H", "g0", "g1"]
    assert "kPluginAbi = 12" in open(os.path.join(ROOT, "socp_amd", "csrc", "launch.hpp")).read()
    out = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--help"], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert "--extrema-out" in out and "--extrema-what" in out


# ---- rows on the CPU oracle: the loop of Lane::integrate, u and H at every row ------------------------------------------------

def oracle_rows(o, t1, t2, X0, N):
    """Trace-format rows [R][W] (t, X, u, H, 0, 0) of one segment: row 0 = the start, row k = the accumulated time and the state
    after k RK4 steps (dt = (t2 - t1)/N, the last step clamped to t2 - t)."""
    X, t = np.array(X0, dtype=np.float64), np.float64(t1)
    dt = (np.float64(t2) - t) / N
    rows = []

    def keep():
        rows.append(np.concatenate([[t], X, o.control(float(t), X), np.ravel(o.hamiltonian(float(t), X))[:1], [0.0, 0.0]]))
    keep()
    guard = N + 8
    while t < (t2 - dt / 2) and guard > 0:
        guard -= 1
        h = (t2 - t) if (t + dt > t2) else dt
        X = o.rk4_step(float(t), X, float(h))
        t = t + dt
        keep()
    return np.array(rows)


def goddard_rows(N, mu2=1.0):
    from oracle.oracle import Oracle, MODEL_GODDARD
    o = Oracle(MODEL_GODDARD, step_nbr=N)
    o.set_param("mu2", mu2)
    return o, oracle_rows(o, 0.0, GODDARD_TF, np.concatenate([GODDARD_X0_STATE, GODDARD_PSTAR]), N)


def model_rows(name):
    """(model key, S, NU, packed parameters, rows) on the oracle: the nominal Goddard start; the double integrator's and covid19's
    golden solutions of tests/events_cases.py (covid19: its first segment)."""
    if name == "goddard":
        o, rows = goddard_rows(40)
        return "goddard", 14, 3, o.params()[:8], rows
    import events_cases as ec
    if name == "dint":
        c = ec.case("dint_basic")
        z = c["Z"][0]
        return "dint", 12, 3, c["params"], oracle_rows(c["o"], 0.0, z[12], z[:12], c["N"])
    c = ec.case("covid_m20")
    return "covid", 8, 1, c["params"], oracle_rows(c["o"], c["prob"].time[0], c["prob"].time[1], c["Z"][0][:8], c["N"])


@pytest.mark.parametrize("name", ["goddard", "dint", "covid"])
def test_sequential_reduction_equals_argmin_argmax_on_oracle_rows(built, name):
    key, S, NU, params, rows = model_rows(name)
    event, EC = er.EVENT_FN[key]
    assert rows.shape[1] == 1 + S + NU + 1 + 2 and len(rows) > 10
    t, V = er.channels_of_rows(rows, S, NU, event, EC, params)
    assert V.shape[1] == S + NU + 1 + EC and np.all(np.isfinite(V)), "this comparison is for finite data"
    r = er.reference_extrema(rows, S, NU, 7, event, EC, params)
    assert r["count"] == len(rows) and r["nbad"] == 0 and r["sel"].all()
    lo, hi = np.argmin(V, axis=0), np.argmax(V, axis=0)              # the first occurrence
    cols = np.arange(V.shape[1])
    assert np.array_equal(er.u64(r["vmin"]), er.u64(V[lo, cols])) and np.array_equal(er.u64(r["tmin"]), er.u64(t[lo]))
    assert np.array_equal(er.u64(r["vmax"]), er.u64(V[hi, cols])) and np.array_equal(er.u64(r["tmax"]), er.u64(t[hi]))
    moving = np.sum(lo != hi)
    assert moving >= S // 2, "most channels of these rows vary along the segment"


# ---- the conventions, on crafted rows -----------------------------------------------------------------------------------------

NAN = float("nan")
T5 = np.array([0.0, 0.25, 0.5, 0.75, 1.0])
CRAFTED = {
    # channel values of five rows               vmin tmin  vmax tmax
    "tie":          ([1.0, 3.0, 1.0, 3.0, 2.0], 1.0, 0.0, 3.0, 0.25),          # the first attainment wins
    "minus_zero":   ([0.0, -0.0, 0.0, -0.0, 0.0], 0.0, 0.0, 0.0, 0.0),         # -0.0 never displaces +0.0
    "plus_zero":    ([-0.0, 0.0, -0.0, 0.0, -0.0], -0.0, 0.0, -0.0, 0.0),      # nor +0.0 -0.0
    "nan_first":    ([NAN, 1.0, -1.0, 5.0, 0.0], NAN, 0.0, NAN, 0.0),          # a NaN in row 0 stays
    "nan_later":    ([2.0, NAN, 1.0, NAN, 3.0], 1.0, 0.5, 3.0, 1.0),           # a later NaN never displaces anything
    "inf":          ([2.0, np.inf, -np.inf, 1.0, 0.0], -np.inf, 0.5, np.inf, 0.25),
}


def crafted_matrix():
    names = sorted(CRAFTED)
    return names, np.array([CRAFTED[n][0] for n in names]).T


def test_conventions_on_crafted_rows():
    names, V = crafted_matrix()
    vmin, vmax, tmin, tmax = er.reduce_rows(T5, V)
    for c, n in enumerate(names):
        want = CRAFTED[n][1:]
        got = (vmin[c], tmin[c], vmax[c], tmax[c])
        assert np.array_equal(er.u64(got), er.u64(want)), (n, got, want)
    # R = 1: every pair is row 0
    one = er.reduce_rows(T5[3:4], V[3:4])
    assert np.array_equal(er.u64(one[0]), er.u64(V[3])) and np.array_equal(er.u64(one[1]), er.u64(V[3]))
    assert np.all(one[2] == 0.75) and np.all(one[3] == 0.75)
    # nbad: rows with a selected channel that is not finite -- trace-format rows with S = 2, NU = 1: t, x, p, u, H, aux, aux
    rows = np.array([[0.0, 1.0, 2.0, 0.5, 7.0, 0, 0], [0.1, NAN, 2.0, 0.5, 7.0, 0, 0], [0.2, 1.0, 2.0, np.inf, 7.0, 0, 0],
                     [0.3, 1.0, 2.0, 0.5, NAN, 0, 0], [0.4, 1.0, -np.inf, NAN, NAN, 0, 0]])
    want = {0: 2, er.CONTROL: 3, er.HAMILTONIAN: 3, er.CONTROL | er.HAMILTONIAN: 4, 7: 4}    # (no event channels: bit 2 selects nothing)
    for what, bad in want.items():
        r = er.reference_extrema(rows, 2, 1, what)
        assert r["nbad"] == bad and r["count"] == 5, (what, r["nbad"])
        assert r["sel"].tolist() == [True, True, bool(what & 1), bool(what & 2)]


# ---- the instrument: wrong restatements must differ on those rows ---------------------------------------------------------------

def last_attainment(t, V):
    """The LAST row that attains the extremum instead of the first (NaN rows skipped unless row 0 is one)."""
    out = [np.empty(V.shape[1]) for _ in range(4)]
    for c in range(V.shape[1]):
        col = V[:, c]
        if col[0] != col[0]:
            lo = hi = 0
        else:
            ok = np.where(col == col)[0]
            lo = ok[len(ok) - 1 - np.argmin(col[ok][::-1])]
            hi = ok[len(ok) - 1 - np.argmax(col[ok][::-1])]
        out[0][c], out[1][c], out[2][c], out[3][c] = col[lo], col[hi], t[lo], t[hi]
    return tuple(out)


WRONG = {
    "<= for <": lambda t, V: er.reduce_rows(t, V, below=lambda v, b: v <= b, above=lambda v, b: v >= b),
    "a NaN displaces": lambda t, V: er.reduce_rows(t, V, below=lambda v, b: v < b or v != v, above=lambda v, b: v > b or v != v),
    "last attainment": last_attainment,
}


@pytest.mark.parametrize("name", sorted(WRONG))
def test_wrong_restatements_differ_on_the_crafted_rows(name):
    _, V = crafted_matrix()
    right = np.concatenate([er.u64(a) for a in er.reduce_rows(T5, V)])
    wrong = np.concatenate([er.u64(a) for a in WRONG[name](T5, V)])
    assert not np.array_equal(right, wrong), name


def test_packer_leaves_unselected_columns_absent_buffers_and_guards_alone():
    rows = np.array([[0.0, 1.0, 2.0, 0.5, 7.0, 0, 0], [0.1, 3.0, 1.0, 0.25, 8.0, 0, 0]])
    ref = [[er.reference_extrema(rows, 2, 1, er.HAMILTONIAN)]]
    vmin, vmax, tmin, tmax, cnt, bad = er.pack_extrema(ref, times=(True, False), nbad=False)
    def b(v):
        return er.u64([v])[0]
    assert np.array_equal(vmin[:4], [b(1.0), b(1.0), er.SENT, b(7.0)]) and np.all(vmin[4:] == er.SENT) and len(vmin) == 4 + er.GUARD
    assert np.array_equal(vmax[:4], [b(3.0), b(2.0), er.SENT, b(8.0)])
    assert np.array_equal(tmin[:4], [b(0.0), b(0.1), er.SENT, b(0.0)]) and np.all(tmax == er.SENT)
    assert cnt[0] == 2 and np.all(cnt[1:] == er.SENT_I) and np.all(bad == er.SENT_I)


# ---- the figure the feature is for ----------------------------------------------------------------------------------------------

def test_hamiltonian_spread_of_the_nominal_goddard_start(built):
    """max H - min H over the rows of the nominal start (smooth law, mu2 = 1) at N = 10, 100, 1000: printed (and recorded in
    profiles/extrema_cpu_tests.txt); asserted only to be finite and non-negative -- how fast it falls is a measurement."""
    for N in (10, 100, 1000):
        _, rows = goddard_rows(N)
        r = er.reference_extrema(rows, 14, 3, er.HAMILTONIAN)
        h = 14 + 3
        spread = r["vmax"][h] - r["vmin"][h]
        print("goddard nominal start, mu2 = 1, N = %4d: rows %4d  H in [%.17g, %.17g]  spread %.3e  (Hmin at t = %.6f, Hmax at t = %.6f)"
              % (N, r["count"], r["vmin"][h], r["vmax"][h], spread, r["tmin"][h], r["tmax"][h]))
        assert r["count"] == N + 1 and r["nbad"] == 0
        assert np.isfinite(spread) and spread >= 0.0
