"""CPU: (a) the definition of socp_group_batch as tests/group_reference.py restates it, on tables small enough to check by hand;
(b) the header declares the two entry points, the built library exports them and capi wraps them; (c) the sweep tool lists
--roots-out."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

import group_reference as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("socp_group_batch", "socp_group_batch_dev")
NAN, INF = np.nan, np.inf


def col(*values):
    return np.array(values, dtype=np.float64)[:, None]


# ---- (a) ----------------------------------------------------------------------------------------------------------------------

def test_the_relation_is_not_transitive_and_the_first_leader_wins():
    """atol = 1: row 1 is near row 0, row 2 is near row 1 but NOT near row 0 -- it leads a group of its own."""
    r = gr.group_reference(col(0.0, 0.75, 1.5), atol=1.0, rtol=0.0, max_groups=4)
    assert r["label"].tolist() == [0, 0, 1]
    assert r["leader"].tolist() == [0, 2, -1, -1] and r["count"].tolist() == [2, 1, 0, 0]
    assert r["radius"].tolist() == [0.75, 0.0, 0.0, 0.0] and r["summary"].tolist() == [2, 0, 0, 0]
    # first, not nearest: 1.25 is nearer to the leader 1.5 than to the leader 0.25, and joins 0.25
    r = gr.group_reference(col(0.25, 1.5, 1.25), atol=1.0, rtol=0.0, max_groups=4)
    assert r["label"].tolist() == [0, 1, 0] and r["radius"][:2].tolist() == [1.0, 0.0]
    # row order matters: the same rows, reversed
    r = gr.group_reference(col(1.5, 0.75, 0.0), atol=1.0, rtol=0.0, max_groups=4)
    assert r["label"].tolist() == [0, 0, 1] and r["leader"][:2].tolist() == [0, 2]


def test_the_bound_is_inclusive_relative_to_the_leader_and_per_entry():
    e = 2.0 ** -10
    V = np.array([[1.0, -1.0, 0.0], [1.0 + e, -1.0 - e, 0.0], [np.nextafter(1.0 + e, 2.0), -1.0, 0.0], [1.0, -1.0, -0.0], [1.0, -1.0, 5e-324]])
    r = gr.group_reference(V, atol=0.0, rtol=e, max_groups=8)
    assert r["label"].tolist() == [0, 0, 1, 0, 2]          # one entry one ulp out is out; a zero leader entry takes +-0 only
    assert r["radius"][0] == e and r["count"][:3].tolist() == [3, 1, 1]
    # only the first n entries are compared
    V = np.array([[1.0, NAN], [1.0, 7.0], [2.0, NAN]])
    assert gr.group_reference(V, n=1, atol=0.0, rtol=0.0)["label"].tolist() == [0, 0, 1]
    assert gr.group_reference(V, atol=0.0, rtol=0.0)["label"].tolist() == [gr.NOTFINITE, 0, gr.NOTFINITE]


def test_overflow_rows_that_are_not_finite_and_a_mask():
    V = col(0.0, NAN, 10.0, INF, 20.0, 0.5, -INF, 30.0, 10.5)
    r = gr.group_reference(V, atol=1.0, rtol=0.0, max_groups=2)
    assert r["label"].tolist() == [0, -2, 1, -2, -1, 0, -2, -1, 1]
    assert r["leader"].tolist() == [0, 2] and r["count"].tolist() == [2, 2] and r["radius"].tolist() == [0.5, 0.5]
    assert r["summary"].tolist() == [2, 2, 3, 0]
    # the mask comes first: a masked row is neither looked at (NaN) nor a leader (row 0), and keeps no slot
    mask = np.array([0, 0, 1, 1, 1, 1, 1, 0, 1])
    r = gr.group_reference(V, mask=mask, atol=1.0, rtol=0.0, max_groups=2)
    assert r["label"].tolist() == [-3, -3, 0, -2, 1, -1, -2, -3, 0]
    assert r["leader"].tolist() == [2, 4] and r["count"].tolist() == [2, 1] and r["summary"].tolist() == [2, 1, 2, 3]
    # everything masked, and an empty table
    r = gr.group_reference(V, mask=np.zeros(9, dtype=int), max_groups=3)
    assert r["summary"].tolist() == [0, 0, 0, 9] and r["leader"].tolist() == [-1, -1, -1] and r["count"].tolist() == [0, 0, 0]
    r = gr.group_reference(np.zeros((0, 4)), max_groups=3)
    assert r["summary"].tolist() == [0, 0, 0, 0] and len(r["label"]) == 0 and r["radius"].tolist() == [0.0, 0.0, 0.0]


def test_counts_labels_and_leaders_are_consistent_on_a_random_table():
    rng = np.random.default_rng(5)
    roots = rng.standard_normal((7, 5)) * 10.0
    pick = rng.integers(0, 7, 300)
    V = roots[pick] * (1.0 + 1e-9 * rng.standard_normal((300, 5)))
    r = gr.group_reference(V, rtol=1e-6, max_groups=16)
    G = int(r["summary"][0])
    assert G == 7 and np.array_equal(np.bincount(r["label"], minlength=16), r["count"])
    assert np.all(r["label"][r["leader"][:G]] == np.arange(G)) and np.all(np.diff(r["leader"][:G]) > 0)
    # the grouping is the partition by root
    assert all(len(set(pick[r["label"] == g].tolist())) == 1 for g in range(G))
    assert 0 < r["radius"][:G].max() < 1e-6 * np.abs(roots).max()


# ---- (b) ----------------------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_group_entry_points():
    from socp_amd import capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "socp_hip.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"^int %s\s*\(socp_ctx \*ctx, int B, int n, int ld, const double \*" % s, text, flags=re.M), s
    for name, value in (("OVERFLOW", -1), ("NOTFINITE", -2), ("MASKED", -3)):
        assert re.search(r"#define SOCP_GROUP_%s\s+%d\b" % (name, value), text), name
    lib = ctypes.CDLL(capi.LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    # without a context nothing runs
    L = capi.lib()
    assert len(L.socp_group_batch.argtypes) == 14 and len(L.socp_group_batch_dev.argtypes) == 14
    assert L.socp_group_batch(None, 0, 1, 1, None, None, 0.0, 0.0, 1, None, None, None, None, None) == capi.ERR_ARG


def test_capi_wraps_the_group_entry_points():
    from socp_amd import capi
    assert callable(getattr(capi.Context, "group_batch", None)) and callable(getattr(capi.Context, "group_batch_dev", None))
    assert (capi.GROUP_OVERFLOW, capi.GROUP_NOTFINITE, capi.GROUP_MASKED) == (gr.OVERFLOW, gr.NOTFINITE, gr.MASKED) == (-1, -2, -3)


# ---- (c) ----------------------------------------------------------------------------------------------------------------------

def test_sweep_tool_lists_roots_out_and_checks_its_arguments():
    run = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    for opt in ("--roots-out", "--roots-rtol", "--roots-atol", "--roots-max"):
        assert opt in run.stdout, opt
    # argument errors come before any device work: exit status 2 on a machine without a GPU too
    for bad_args in (["--roots-max", "0"], ["--roots-rtol", "-1"], ["--roots-atol", "nan"]):
        bad = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--roots-out", "x"] + bad_args, cwd=ROOT, capture_output=True, text=True,
                             timeout=120)
        assert bad.returncode == 2 and bad_args[0] in bad.stderr, (bad_args, bad.stderr[-500:])
