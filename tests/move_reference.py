"""Test infrastructure: the numpy restatement of the batched Move(tf) / re-grid (socp_move_batch, socp_regrid_batch) on the CPU
oracle -- capi.move_segment for the selection rule (shooting.cpp:407-424), Oracle.traj for model::ComputeTraj (:433), and the pack
rule of shooting.cpp:228-243.  What the GPU tests compare with; tests/test_move_batch_cpu.py pins it to OracleShooting.move and to
the re-grid goddard_test_flow builds.  Not product code."""
import numpy as np

from oracle.oracle import FREE


def regrid_num_param(s, mode_t2):
    """n2 = s M2 + #FREE(mode_t2)."""
    return s * (len(mode_t2) - 1) + sum(1 for m in mode_t2 if m == FREE)


def move(orc, tl, z, s, q):
    """Move(q) on the stored solution z with timeline tl: (state, target time)."""
    from socp_amd import capi
    seg, target = capi.move_segment(tl, q)
    return orc.traj(float(tl[seg]), np.asarray(z[s * seg:s * seg + s], dtype=np.float64), float(target)), target


def regrid(orc, tl, z, s, mode_t2, T2):
    """One solution onto a new structure: dict(z[n2], time[M2+1], xnode[M2+1][s])."""
    M2 = len(mode_t2) - 1
    T2 = np.asarray(T2, dtype=np.float64)
    X = np.stack([move(orc, tl, z, s, T2[j])[0] for j in range(M2 + 1)])
    z2 = np.concatenate([X[:M2].ravel(), [T2[j] for j in range(M2 + 1) if mode_t2[j] == FREE]])
    assert len(z2) == regrid_num_param(s, mode_t2)
    return dict(z=z2, time=T2.copy(), xnode=X)
