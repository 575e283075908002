"""CPU: the definition behind socp_move_batch / socp_regrid_batch and its surface.
(a) capi.move_segment -- the selection rule of shooting::Move(tf) -- against OracleShooting.move on the golden stage-3 solution of
    the testGoddard flow, for queries on nodes, inside segments, out of range and NaN; (b) tests/move_reference.py -- the numpy
    restatement the GPU tests compare with -- reproduces the re-grid goddard_test_flow builds before its stage 4, bit for bit;
(c) the symbols are declared, exported and wrapped, socp_regrid_num_param gives 87 for the stage-4 structure, and the sweep tool
    lists the new switches."""
import json
import os
import re
import subprocess
import sys

import numpy as np

import move_reference
from flow_oracle import OracleShooting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "goddard_flow.json")))
SYMBOLS = ("socp_move_batch_dev", "socp_move_batch", "socp_move_batch_blocks", "socp_regrid_num_param", "socp_regrid_batch_dev",
           "socp_regrid_batch_blocks")
M, S = 6, 14


def stage3_shooting():
    """OracleShooting as goddard_test_flow holds it after its mu2 continuation: KD = 310, mu2 = 0.2, the golden stage-3 unknowns."""
    from oracle.oracle import Oracle, MODEL_GODDARD, FREE
    z = np.array(GOLD["goddard_N10_M6"][2]["z"])
    assert GOLD["goddard_N10_M6"][2]["stage"] == "mu2_continuation" and len(z) == 85
    o = Oracle(MODEL_GODDARD, step_nbr=10)
    o.set_param("KD", 310.0)
    o.set_param("mu2", 0.2)
    sh = OracleShooting(o, M)
    mode_xf = np.zeros(7, dtype=np.int32)
    mode_xf[3:7] = FREE
    sh.set_mode_final(FREE, mode_xf)
    Xi = np.array([0.999949994, 1e-4, 0.01, 1e-10, 1e-10, 1e-10, 1.0] + [0.1] * 7)
    Xf = np.zeros(14)
    Xf[0] = 1.01
    sh.init_uniform(0.0, Xi, 0.1, Xf)
    sh.z = z.copy()
    return o, sh, z, mode_xf


def stage4_structure(mode_xf):
    from oracle.oracle import FIXED, FREE, CONTINUOUS
    mode_t = [FIXED, CONTINUOUS, FREE, CONTINUOUS, FREE, CONTINUOUS, FREE]
    mode_x = np.full((M + 1, 7), CONTINUOUS, dtype=np.int32)
    mode_x[0] = FIXED
    mode_x[M] = mode_xf
    return mode_t, mode_x


def stage4_times(tf):
    s1, s2 = 0.0227, 0.08
    return np.array([0.0, s1 / 2, s1, (s2 + s1) / 2, s2, (s2 + tf) / 2, tf])


def test_move_segment_against_the_oracle_move(built):
    from socp_amd import capi
    o, sh, z, _ = stage3_shooting()
    tf = z[-1]
    assert abs(tf - 0.231085518) < 1e-9
    tl = sh.timeline()
    assert tl[0] == 0.0 and tl[M] == tf
    queries = [0.0, 0.01135, 0.0227, 0.05135, 0.08, (0.08 + tf) / 2, tf, -1.0, 1.0, tl[2], float("nan")]
    want_seg = [0, 0, 0, 1, 2, 4, 5, 5, 5, 1, 5]
    want_target = queries[:7] + [tf, tf, tl[2], tf]
    for q, ws, wt in zip(queries, want_seg, want_target):
        seg, target = capi.move_segment(tl, q)
        assert (seg, target) == (ws, wt), (q, seg, target)
        X = o.traj(tl[seg], z[S * seg:S * seg + S], target)
        assert np.array_equal(X, sh.move(q)), q
        Xr, tr = move_reference.move(o, tl, z, S, q)
        assert tr == wt and np.array_equal(Xr, X), q
    # q == t0: a zero-length integration returns the first node bit for bit; an interior node time integrates the previous segment
    assert np.array_equal(sh.move(0.0), z[:S])
    assert not np.array_equal(sh.move(tl[2]), z[2 * S:3 * S])
    # a disordered or NaN timeline: the search stops at the first node time that is not below the target, and never past M - 1
    assert capi.move_segment([0.0, 1.0, 5.0, 2.0], 4.0) == (1, 2.0)
    assert capi.move_segment([0.0, 1.0, 5.0, 6.0], 5.5) == (2, 5.5)
    assert capi.move_segment([0.0, float("nan"), 2.0, 3.0], 2.5) == (0, 2.5)
    seg, target = capi.move_segment([0.0, 1.0, 2.0, float("nan")], 1.5)
    assert seg == 0 and target != target


def test_regrid_restatement_reproduces_the_flows_own_regrid(built):
    o, sh, z, mode_xf = stage3_shooting()
    tl = sh.timeline()
    # testGoddard.cpp:115-145 / goddard_test_flow, on the oracle's own objects
    vt, vX = sh.get_solution()
    T2 = stage4_times(vt[M])
    vX2 = np.stack([sh.move(t) for t in T2])
    mode_t2, mode_x2 = stage4_structure(mode_xf)
    got = move_reference.regrid(o, tl, z, S, mode_t2, T2)
    sh.set_mode(mode_t2, mode_x2)
    sh.init_nodes(T2, vX2)
    assert sh.n == 87 == move_reference.regrid_num_param(S, mode_t2)
    assert np.array_equal(got["z"], sh.z) and np.array_equal(got["time"], sh.time) and np.array_equal(got["xnode"], sh.X)
    assert np.array_equal(got["z"][84:], T2[[2, 4, 6]])


def test_symbols_declared_exported_and_wrapped():
    from socp_amd import capi
    header = open(os.path.join(ROOT, "include", "socp_hip.h")).read()
    L = capi.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(L, name), name
    assert re.search(r"socp_move_batch_dev\(socp_ctx \*ctx, int B, const double \*d_Z, int K, const double \*d_tq, double \*d_Xq, double \*d_tout\)",
                     header)
    assert re.search(r"socp_regrid_num_param\(const socp_ctx \*ctx, int M2, const int \*mode_t2\)", header)
    for name in ("move_batch_dev", "move_batch", "regrid_num_param", "regrid_batch_dev", "regrid_batch"):
        assert callable(getattr(capi.Context, name)), name
    assert callable(capi.move_segment)
    assert len(L.socp_move_batch_dev.argtypes) == 7 and len(L.socp_move_batch_blocks.argtypes) == 11
    assert len(L.socp_regrid_batch_dev.argtypes) == 8 and len(L.socp_regrid_batch_blocks.argtypes) == 12
    # n2 of the stage-4 structure: through a context where a device is present, else the formula alone
    mode_t2 = [capi.FIXED, capi.CONTINUOUS, capi.FREE, capi.CONTINUOUS, capi.FREE, capi.CONTINUOUS, capi.FREE]
    assert move_reference.regrid_num_param(S, mode_t2) == 87
    try:
        ctx = capi.Context(capi.MODEL_GODDARD)
    except capi.SocpError as exc:
        assert exc.code == capi.ERR_NO_DEVICE
        return
    assert ctx.regrid_num_param(mode_t2) == 87
    ctx.close()


def test_sweep_tool_lists_the_regrid_switches():
    out = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "--regrid-segments" in out.stdout and "--regrid-out" in out.stdout
