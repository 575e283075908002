"""CPU: the definition of socp_events_batch (tests/events_reference.py) on the golden stage-3 solution of the testGoddard flow,
the margin condition the GPU event tests rest on, and the surface of the feature (header, library, bindings, sweep tool).

(a) The issue states the events of the golden row as it measured them: segment 0, step 1, id +1 at 0.005012714637908262 and
segment 3, step 0, id +2 at 0.11913872605795654 (N = 10, R = 2).  Re-derived here, the first is reproduced bit for bit on every
timeline.  The second is reproduced bit for bit when the node times are formed as np.linspace(0, tf, 7) (node 3 at
0.11554275901527253); on the SHOOTING timeline -- ta + (k - a)*(tb - ta)/(b - a), shooting.cpp:1586-1613, what the residual and
therefore socp_events_batch use -- node 3 is 0.11554275901527251, two units in the last place lower, the located length th inside
the step is the same (the smooth law does not read t), and the event time comes out one unit lower, 0.11913872605795653.  Both are
asserted below; test_gpu_events_batch.py compares the device against the shooting timeline's value."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import events_cases as ec
from conftest import goddard_c1_problem
from events_reference import goddard_event, pack_events, reference_events, reference_events_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_SATURATION, T_OFF = 0.005012714637908262, 0.11913872605795654          # the issue's figures, N = 10, R = 2
T_OFF_SHOOTING_TIMELINE = 0.11913872605795653
T_SATURATION_FINE, T_OFF_FINE = 0.0050123875, 0.1191387317               # N = 1000, R = 3


def flat(rows):
    return [(i, ev["k"], ev["id"], float(ev["t"])) for i, seg in enumerate(rows) for ev in seg]


def golden_rows_on(times, N, R):
    """The golden row's segments integrated between the given node times (7 of them) on the oracle."""
    o = ec.goddard_oracle(N)
    z, p = ec.goddard_stage3_row(), o.params()
    step = lambda t, X, h: o.rk4_step(float(t), X, float(h))                  # noqa: E731
    return [reference_events(step, lambda X, c: goddard_event(p, X, c), times[i], times[i + 1], z[14 * i:14 * i + 14], N, [0, 0],
                             [-0.4, 0.0], R) for i in range(6)]


def test_golden_row_events_are_the_issue_s(built):
    z = ec.goddard_stage3_row()
    got = flat(golden_rows_on(np.linspace(0.0, z[84], 7), 10, 2))
    print("golden row, N = 10, R = 2, uniform node times:", got)
    assert got == [(0, 1, 1, T_SATURATION), (3, 0, 2, T_OFF)], got


def test_golden_row_events_on_the_shooting_timeline(built):
    o = ec.goddard_oracle(10)
    prob, _ = goddard_c1_problem(o)
    z = ec.goddard_stage3_row()
    tl = o.timeline(prob, z)
    assert tl[3] == 0.11554275901527251 and np.linspace(0.0, z[84], 7)[3] == 0.11554275901527253
    rows = reference_events_batch(o, prob, z[None], 10, [0, 0], [[-0.4, 0.0]], 2)[0]
    got = flat(rows)
    print("golden row, N = 10, R = 2, shooting timeline:", got)
    assert got == [(0, 1, 1, T_SATURATION), (3, 0, 2, T_OFF_SHOOTING_TIMELINE)], got
    assert got == flat(golden_rows_on(tl, 10, 2))
    assert abs(T_OFF_SHOOTING_TIMELINE - T_OFF) == np.spacing(T_OFF)
    # the state at an event sits on the level to the refinement's accuracy: two false-position steps take the 0.1 .. 0.4 the
    # channel moves over such a step down to 1e-5 and below (linear interpolation alone leaves 1e-2)
    for seg in rows:
        for ev in seg:
            g = goddard_event(o.params(), ev["X"], 0) - [-0.4, 0.0][ev["e"]]
            assert abs(g) < 1e-4, (ev["t"], g)


def test_golden_row_events_at_a_thousand_steps(built):
    o = ec.goddard_oracle(1000)
    prob, _ = goddard_c1_problem(o)
    got = flat(reference_events_batch(o, prob, ec.goddard_stage3_row()[None], 1000, [0, 0], [[-0.4, 0.0]], 3)[0])
    print("golden row, N = 1000, R = 3:", got)
    assert [(g[0], g[2]) for g in got] == [(0, 1), (3, 2)]
    assert abs(got[0][3] - T_SATURATION_FINE) <= 1e-9 and abs(got[1][3] - T_OFF_FINE) <= 1e-9
    # not the reference's hand-picked switching times of the next structure (testGoddard.cpp:117-118)
    assert abs(got[0][3] - 0.0227) > 0.01 and abs(got[1][3] - 0.08) > 0.03


def test_linear_interpolation_is_refine_zero(built):
    o = ec.goddard_oracle(10)
    prob, _ = goddard_c1_problem(o)
    z = ec.goddard_stage3_row()
    r0 = flat(reference_events_batch(o, prob, z[None], 10, [0, 0], [[-0.4, 0.0]], 0)[0])
    r2 = flat(reference_events_batch(o, prob, z[None], 10, [0, 0], [[-0.4, 0.0]], 2)[0])
    assert [g[:3] for g in r0] == [g[:3] for g in r2]
    assert all(0.0 < abs(a[3] - b[3]) < 2e-4 for a, b in zip(r0, r2)), (r0, r2)      # inside one step of 3.85e-3


@pytest.mark.parametrize("name", sorted(ec.CASES))
def test_margin_condition_of_the_gpu_inputs(built, name):
    """min |channel - level| over every step end of every row the GPU tests use is > 1e-6: no flavour can flip a sign."""
    m = ec.margin(name)
    rows = ec.reference(name, 2)
    per_watch = [sum(1 for row in rows for seg in row for ev in seg if ev["e"] == e) for e in range(len(ec.case(name)["chan"]))]
    print("%s: margin %.3e, events per watch %s" % (name, m, per_watch))
    assert m > 1e-6
    assert all(k >= 1 for k in per_watch), "every watch of the GPU inputs has a crossing"
    assert all(np.all(np.isfinite(ev["X"])) and np.isfinite(ev["t"]) for row in rows for seg in row for ev in seg)


def test_the_gpu_inputs_hold_the_shapes_their_tests_are_about(built):
    count = lambda name: np.array([[len(seg) for seg in row] for row in ec.reference(name, 2)])      # noqa: E731
    assert count("goddard_b130").max() == 2, "a segment with two events: what cap = 1 cuts"
    assert np.all(count("goddard_degenerate")[:, 1:3] == 0) and np.all(count("goddard_degenerate")[:, 0] >= 1)
    assert len(np.unique(ec.case("goddard_blocks")["levels"][:, 0])) == 130
    covid = ec.reference("covid_m20", 2)
    assert {ev["e"] for row in covid for seg in row for ev in seg} == {0, 1}


def test_pack_events_counts_all_and_stores_the_first_cap():
    rows = [[[dict(t=1.0, id=1, X=np.ones(2)), dict(t=2.0, id=-2, X=np.full(2, 2.0))], []]]
    t, ident, count, X = pack_events(rows, 1, 2)
    assert count.tolist() == [[2, 0]] and t[0, 0, 0] == 1.0 and ident[0, 0, 0] == 1 and np.isnan(t[0, 1, 0]) and np.all(X[0, 0, 0] == 1.0)


# ---- (c) surface ------------------------------------------------------------------------------------------------------------

SYMBOLS = ("socp_ctx_event_channels", "socp_events_batch_dev", "socp_events_batch", "socp_events_batch_blocks")


def test_symbols_are_declared_exported_and_wrapped():
    from socp_amd import capi
    header = open(os.path.join(ROOT, "include", "socp_hip.h")).read()
    for name in SYMBOLS:
        assert "int %s(" % name in header, name
    lib = C.CDLL(capi.LIB_PATH)
    for name in SYMBOLS:
        assert getattr(lib, name) is not None
    source = open(os.path.join(ROOT, "socp_amd", "capi.py")).read()
    for name in SYMBOLS:
        assert "L.%s.argtypes" % name in source, name
    for method in ("event_channels", "events_batch_dev", "events_batch"):
        assert callable(getattr(capi.Context, method))
    assert "kPluginAbi = 9" in open(os.path.join(ROOT, "socp_amd", "csrc", "launch.hpp")).read()
    assert "kEventChannels" in open(os.path.join(ROOT, "include", "socp_plugin.h")).read()
    assert "kEventChannels" not in open(os.path.join(ROOT, "tests", "plugin", "lqr1d_plugin.hip")).read(), "the example plugin stays without the trait"


def test_merge_events_sorts_across_segments():
    from socp_amd import capi
    nan = np.nan
    t = np.array([[[0.30, 0.10], [0.20, nan], [nan, nan]],
                  [[0.50, nan], [nan, nan], [0.40, 0.45]]])
    ident = np.array([[[2, -1], [1, 0], [0, 0]],
                      [[-2, 0], [0, 0], [1, 2]]], dtype=np.int32)
    count = np.array([[2, 1, 0], [1, 0, 3]], dtype=np.int32)                 # the last segment had 3 events, cap stored 2
    merged = capi.merge_events(t, ident, count)
    assert len(merged) == 2
    assert merged[0][0].tolist() == [0.10, 0.20, 0.30] and merged[0][1].tolist() == [-1, 1, 2]
    assert merged[1][0].tolist() == [0.40, 0.45, 0.50] and merged[1][1].tolist() == [1, 2, -2]
    empty = capi.merge_events(np.full((1, 2, 4), nan), np.zeros((1, 2, 4), dtype=np.int32), np.zeros((1, 2), dtype=np.int32))
    assert len(empty) == 1 and len(empty[0][0]) == 0 and len(empty[0][1]) == 0


def test_sweep_tool_lists_the_new_switches():
    run = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "--events-out" in run.stdout and "--events-refine" in run.stdout and "socp_events_batch" in run.stdout
    bad = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--model", "interceptor", "--events-out", "x"], cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--events-out" in bad.stderr and "interceptor" in bad.stderr
