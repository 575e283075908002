"""CPU: the definition of socp_observe_batch as tests/observe_reference.py restates it -- (0) the surface exists; (1) the fuel check:
the trapezoid integral of Goddard's fuel_rate along the CPU oracle's stride-1 rows against the mass those rows lose; (2) hand-made
rows that pin the rules of the reduction; (3) the clearance on hand-made points; (4) the instrument: wrong restatements differ from
the right one on those inputs.  No GPU; the library is only asked for its symbols.

Measured (profiles/observe_cpu_tests.txt): nominal Goddard start, mu2 = 1, M = 1, [0, 0.2640825]: |integral of fuel_rate - mass
drop| = 2.298e-04 at N = 50, 7.643e-05 at N = 100 and 1.158e-05 at N = 200 (burnt mass 0.4331): it shrinks at each doubling, by
3.01 and then 6.60 -- not the steady 4 of a smooth integrand: the saturation kinks of the thrust fall inside a step."""
import os
import subprocess
import sys

import numpy as np
import pytest

import observe_reference as obr
from test_extrema_cpu import goddard_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("socp_observe_batch", "socp_observe_batch_dev", "socp_observe_batch_blocks", "socp_ctx_has_observe", "socp_ctx_observables",
           "socp_ctx_observable_name")
NAN, INF = float("nan"), float("inf")


def bits(*arrays):
    return np.concatenate([obr.u64(np.ravel(a)) for a in arrays])


def test_library_header_python_layer_plugin_and_sweep_tool_have_the_feature():
    """Fails without the feature."""
    from socp_amd import capi
    from test_capi_symbols import declared_functions
    declared = declared_functions()
    L = capi.lib()
    for name in SYMBOLS:
        assert name in declared, name + " is not declared in include/"
        assert hasattr(L, name), name + " is not exported"
    assert len(L.socp_observe_batch_dev.argtypes) == 10 and len(L.socp_observe_batch.argtypes) == 10
    assert len(L.socp_observe_batch_blocks.argtypes) == 14
    for name in ("has_observe", "observable_names", "observe_batch_dev", "observe_batch"):
        assert callable(getattr(capi.Context, name)), name
    assert "kPluginAbi = 14" in open(os.path.join(ROOT, "socp_amd", "csrc", "launch.hpp")).read()
    for doc in ("include/socp_plugin.h", "socp_amd/csrc/plugin_impl.hpp"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "kObservables" in text and "kObservableNames" in text and "observe(" in text, doc
    assert os.path.exists(os.path.join(ROOT, "tests", "plugin", "osc1d_observe_plugin.hip"))
    out = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--help"], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert "--observe-out" in out


# ---- (1) the fuel check -----------------------------------------------------------------------------------------------------------

def test_integral_of_fuel_rate_approaches_the_mass_drop(built):
    """fuel_rate = b |u| and row 6 of the right-hand side is -b |u|: the trapezoid integral over the rows and the mass drop of the
    same rows, X[6](t1) - X[6](t2), differ by the quadrature error of two different rules.  Asserted: it shrinks at each doubling
    of N.  The ratio (about 4 for a smooth law) is printed, not asserted."""
    errs = []
    for N in (50, 100, 200):
        o, rows = goddard_rows(N)
        r = obr.reference_observe("goddard", rows, o.params()[:8])
        k = obr.OBSERVE["goddard"][3].index("fuel_rate")
        drop = rows[0, 1 + 6] - rows[-1, 1 + 6]
        err = abs(r["integral"][k] - drop)
        errs.append(err)
        print("goddard nominal start, mu2 = 1, N = %3d: rows %3d  integral of fuel_rate %.12e  mass drop %.12e  |difference| %.3e%s"
              % (N, r["count"], r["integral"][k], drop, err, "  ratio %.2f" % (errs[-2] / err) if len(errs) > 1 else ""))
        print("    peak drag %.6e at t = %.6f, peak drag_acc %.6e, peak r %.9f, peak v %.6e at t = %.6f"
              % (r["ymax"][3], r["tmax"][3], r["ymax"][4], r["ymax"][0], r["ymax"][1], r["tmax"][1]))
        assert r["count"] == N + 1 and r["nbad"] == 0 and drop > 0.0 and r["integral"][k] > 0.0
        # r and v carry the bits of the norms, whatever the order of the rows
        assert np.array_equal(obr.u64(r["ymax"][0]), obr.u64(np.max(np.sqrt(rows[:, 1]**2 + rows[:, 2]**2 + rows[:, 3]**2))))
    assert errs[1] < errs[0] and errs[2] < errs[1], errs


# ---- (2) the rules, on hand-made rows ---------------------------------------------------------------------------------------------

T5 = np.array([0.0, 0.25, 0.5, 1.0, 1.5])
CRAFTED = {
    # values of five rows                        ymin  tmin  ymax  tmax  integral
    "tie":        ([1.0, 3.0, 1.0, 3.0, 2.0],    1.0,  0.0,  3.0,  0.25, 0.5 + 0.5 + 1.0 + 1.25),     # the first attainment wins
    "minus_zero": ([0.0, -0.0, 0.0, -0.0, 0.0],  0.0,  0.0,  0.0,  0.0,  0.0),                         # -0.0 never displaces +0.0
    "plus_zero":  ([-0.0, 0.0, -0.0, 0.0, -0.0], -0.0, 0.0,  -0.0, 0.0,  0.0),                         # nor +0.0 -0.0; the sum starts at +0.0
    "nan_first":  ([NAN, 1.0, -1.0, 5.0, 0.0],   NAN,  0.0,  NAN,  0.0,  NAN),                         # a NaN in row 0 stays; it enters the sum
    "nan_later":  ([2.0, NAN, 1.0, NAN, 3.0],    1.0,  0.5,  3.0,  1.5,  NAN),                         # a later NaN displaces nothing
    "inf":        ([2.0, INF, 4.0, 1.0, 0.0],    0.0,  1.5,  INF,  0.25, INF),                         # an infinite value enters the sum
    "ramp":       ([0.0, 1.0, 2.0, 4.0, 6.0],    0.0,  0.0,  6.0,  1.5,  0.125 + 0.375 + 1.5 + 2.5),
}


def crafted_matrix():
    names = sorted(CRAFTED)
    return names, np.array([CRAFTED[n][0] for n in names]).T


def test_rules_on_crafted_rows():
    names, Y = crafted_matrix()
    r = obr.reduce_rows(T5, Y)
    for c, n in enumerate(names):
        want = CRAFTED[n][1:]
        got = (r["ymin"][c], r["tmin"][c], r["ymax"][c], r["tmax"][c], r["integral"][c])
        assert np.array_equal(obr.u64(got), obr.u64(want)), (n, got, want)
    assert r["count"] == 5 and r["nbad"] == 3            # rows 0, 1 and 3 hold a NaN; row 1 holds the infinity as well and counts once
    assert obr.reduce_rows(T5, Y[:, [names.index("ramp")]])["nbad"] == 0
    assert obr.reduce_rows(T5, Y[:, [names.index("inf")]])["nbad"] == 1
    # a single-row segment: every pair is row 0 and the integral is +0.0
    one = obr.reduce_rows(T5[3:4], Y[3:4])
    assert np.array_equal(obr.u64(one["ymin"]), obr.u64(Y[3])) and np.array_equal(obr.u64(one["ymax"]), obr.u64(Y[3]))
    assert np.all(one["tmin"] == 1.0) and np.all(one["tmax"] == 1.0) and one["count"] == 1
    assert np.array_equal(obr.u64(one["integral"]), obr.u64(np.zeros(len(names))))
    # the operation order of the sum: I + (0.5 w) s with s = y_k + y_{k-1}, every operation rounding once
    t = np.array([0.0, 0.1, 0.3, 0.7])
    y = np.array([[0.1], [0.2], [0.7], [1e-17]])
    I = np.float64(0.0)
    for k in (1, 2, 3):
        I = I + (np.float64(0.5) * (t[k] - t[k - 1])) * (y[k, 0] + y[k - 1, 0])
    assert np.array_equal(obr.u64(obr.reduce_rows(t, y)["integral"]), obr.u64([I]))


def test_nbad_counts_rows_not_values():
    Y = np.array([[1.0, 2.0], [NAN, INF], [1.0, -INF], [1.0, 2.0]])
    assert obr.reduce_rows(np.arange(4.0), Y)["nbad"] == 2


# ---- (3) the clearance ------------------------------------------------------------------------------------------------------------

BOX = [1.0, 10.0, 20.0, 30.0, 2.0, 3.0, 4.0]              # type 1: centre (10, 20, 30), half-widths (2, 3, 4)
ELL = [0.0, -5.0, 0.0, 0.0, 2.0, 1.0, 4.0]                # type 0: centre (-5, 0, 0), radii (2, 1, 4)


def test_clearance_on_crafted_points():
    cl = obr.clearance
    # a box: inside (negative: the largest of the three signed distances), on a face (zero), outside
    assert cl(10.5, 20.0, 30.0, [BOX]) == -1.5 and cl(11.0, 22.5, 30.0, [BOX]) == -0.5 and cl(9.0, 21.0, 33.5, [BOX]) == -0.5
    assert cl(12.0, 20.0, 30.0, [BOX]) == 0.0 and cl(8.0, 23.0, 26.0, [BOX]) == 0.0
    assert cl(15.0, 20.0, 30.0, [BOX]) == 3.0 and cl(10.0, 20.0, 36.5, [BOX]) == 2.5 and cl(5.0, 10.0, 30.0, [BOX]) == 7.0
    # an ellipsoid: d - d / sqrt(sum (h / rad)^2) along the axes is |h| - rad
    assert cl(-5.0, 0.5, 0.0, [ELL]) == -0.5 and cl(-4.0, 0.0, 0.0, [ELL]) == -1.0
    assert cl(-3.0, 0.0, 0.0, [ELL]) == 0.0 and cl(-5.0, 0.0, -4.0, [ELL]) == 0.0
    assert cl(-5.0, 3.0, 0.0, [ELL]) == 2.0 and cl(-5.0, 0.0, 6.0, [ELL]) == 2.0
    off = cl(-3.0, 1.0, 2.0, [ELL])
    hx, hy, hz = 2.0, 1.0, 2.0
    d = np.sqrt(np.float64(hx*hx + hy*hy + hz*hz))
    assert off == d - d / np.sqrt(np.float64(1.0 + 1.0 + 0.25)) and off > 0.0
    # the centre of an ellipsoid: 0 / 0, a NaN level that displaces nothing -- alone it leaves +inf, beside a box the box's level
    assert cl(-5.0, 0.0, 0.0, [ELL]) == np.inf
    assert cl(-5.0, 0.0, 0.0, [ELL, BOX]) == cl(-5.0, 0.0, 0.0, [BOX]) == cl(-5.0, 0.0, 0.0, [BOX, ELL]) == 26.0
    # an empty table
    assert cl(1.0, 2.0, 3.0, np.zeros((0, 7))) == np.inf
    # two overlapping boxes: the smaller level, whatever the table order (the minimum is strict: a tie keeps the first, the same value)
    big = [1.0, 10.0, 20.0, 30.0, 5.0, 5.0, 5.0]
    for p, want in (((10.5, 20.0, 30.0), -4.5), ((13.0, 20.0, 30.0), -2.0), ((16.0, 20.0, 30.0), 1.0)):
        assert cl(*p, [BOX, big]) == cl(*p, [big, BOX]) == want
    assert cl(12.0, 20.0, 30.0, [BOX, BOX]) == 0.0
    # the observable reads the position from the state
    X = np.zeros(12)
    X[:6] = [15.0, 20.0, 30.0, 3.0, 4.0, 12.0]
    y = obr.vtol_observe(None, 0.0, X, np.array([0.0, 3.0, 4.0]), np.array([BOX, ELL]))
    assert y == [13.0, 5.0, 3.0]


# ---- (4) the instrument: wrong restatements must differ ---------------------------------------------------------------------------

def rectangle(I, w, y, y_prev):
    return I + w * y_prev


def box_without_fabs(px, py, pz, o):
    m = (px - o[1]) - o[4]
    b = (py - o[2]) - o[5]
    c = (pz - o[3]) - o[6]
    return max(m, b, c)


def ellipsoid_two_terms(px, py, pz, o):
    """The radius of the map's gradient (no z term) in place of the value's."""
    hx, hy, hz = px - o[1], py - o[2], pz - o[3]
    d = np.sqrt(hx*hx + hy*hy + hz*hz)
    with np.errstate(all="ignore"):
        return d - d / np.sqrt(hx*hx / o[4] / o[4] + hy*hy / o[5] / o[5])


POINTS = [(10.5, 20.0, 30.0), (9.0, 21.0, 33.5), (5.0, 10.0, 30.0), (-3.0, 1.0, 2.0), (-5.0, 0.5, 3.0), (-6.0, 0.25, -1.0)]


def reduction_bits(**kw):
    _, Y = crafted_matrix()
    r = obr.reduce_rows(T5, Y, **kw)
    return bits(*[r[k] for k in obr.KEYS])


def clearance_bits(**kw):
    with np.errstate(all="ignore"):
        return bits([obr.clearance(*p, [BOX, ELL], **kw) for p in POINTS])


WRONG = {
    "rectangle rule": (reduction_bits, dict(quadrature=rectangle)),
    "<= for <": (reduction_bits, dict(below=lambda v, b: v <= b, above=lambda v, b: v >= b)),
    "a NaN displaces": (reduction_bits, dict(below=lambda v, b: v < b or v != v, above=lambda v, b: v > b or v != v)),
    "clearance without fabs": (clearance_bits, dict(box=box_without_fabs)),
    "two-term ellipsoid radius": (clearance_bits, dict(ellipsoid=ellipsoid_two_terms)),
    "clearance keeps the last level": (clearance_bits, dict(below=lambda v, b: True)),
}


@pytest.mark.parametrize("name", sorted(WRONG))
def test_wrong_restatements_differ_on_the_crafted_inputs(name):
    fn, kw = WRONG[name]
    with np.errstate(all="ignore"):
        assert not np.array_equal(fn(), fn(**kw)), name


def test_packer_leaves_absent_buffers_and_guards_alone():
    ref = [[obr.reduce_rows(np.array([0.0, 0.5]), np.array([[1.0, 4.0], [3.0, 2.0]]))]]
    ymin, ymax, tmin, tmax, integral, cnt, bad = obr.pack_observe(ref, given=(True, False, True), nbad=False)

    def b(v):
        return obr.u64([v])[0]
    assert np.array_equal(ymin[:2], [b(1.0), b(2.0)]) and np.all(ymin[2:] == obr.SENT) and len(ymin) == 2 + obr.GUARD
    assert np.array_equal(ymax[:2], [b(3.0), b(4.0)]) and np.array_equal(tmin[:2], [b(0.0), b(0.5)]) and np.all(tmax == obr.SENT)
    assert np.array_equal(integral[:2], [b(1.0), b(1.5)])
    assert cnt[0] == 2 and np.all(cnt[1:] == obr.SENT_I) and np.all(bad == obr.SENT_I)
