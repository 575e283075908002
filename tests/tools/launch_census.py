#!/usr/bin/env python3
"""Which kernel every entry point launches: a plain driver (no timing, nothing asserted) to be run under a kernel trace,

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tests/tools/launch_census.py
    python tests/tools/launch_census.py --names DIR      the trace's kernels in launch order, one per line, with their grid

once on each of two builds of the library (SOCP_LIB_PATH names the other one); the two name sequences must be identical line for
line (profiles/launch_tables_census.txt).  No test can see which Goddard control law a launch took when mu2 > 0 -- the two kernels
agree in every bit there -- so the choice is compared launch by launch.

Goddard, the C1 problem of tests/test_gpu_cost_batch.py (B = 3, 4 steps): integrate_batch, eval_batch (all three quantities),
integrate_dense, residual_batch, fd_jacobian, fd_rows, trace_batch, cost_batch, move_batch, events_batch, regrid_batch (onto two
segments) -- with mu2 = 0 and mu2 = 1, both variants, both integrators (the cost and the events have the fixed-step one only), without
per-problem blocks and with them (so all six _blocks entry points run both ways): socp_problem_blocks_all_smooth 0
(the blocks carry the context's mu2) and 1 (the blocks carry mu2 = 1 whatever the context holds, so the promise is true).  Then
the same calls once per variant for the double integrator (and var_jacobian) and for covid19."""
import argparse
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def names(trace_dir):
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1)))
    for _, name, grid in sorted(rows):
        print("grid %5d  %s" % (grid, name))


def problem_calls(ctx, Z, blocks, fixed=True):
    """Every entry point that reads the shooting problem; blocks: None or (params, time, xnode), one row per row of Z; fixed: the
    context integrates with fixed steps (the cost and the events have that integrator only)."""
    import torch
    from socp_amd import capi
    kw = dict(zip(("params", "time", "xnode"), blocks)) if blocks else {}
    F = ctx.residual_batch_blocks(Z, **kw)
    keep = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in blocks] if blocks else []
    if blocks:        # fd_jacobian / fd_rows have no _blocks form: the blocks are put in force on the device
        ctx._chk(ctx.L.socp_problem_set_blocks_dev(ctx.h, keep[0].data_ptr(), blocks[0].shape[1], keep[1].data_ptr(), keep[2].data_ptr()))
    ctx.fd_jacobian(Z[0], F[0])
    ctx.fd_rows(Z)
    if blocks:
        ctx._chk(ctx.L.socp_problem_set_blocks_dev(ctx.h, None, 0, None, None))
    ctx.trace_batch(Z, stride=2, cap=8, **kw)
    if fixed:
        ctx.cost_batch(Z, xend=True, **kw)
    tl = np.stack([ctx.timeline(z) for z in Z])
    ctx.move_batch(Z, 0.5 * (tl[:, :-1] + tl[:, 1:]), **kw)
    if fixed and ctx.event_channels() > 0:
        ctx.events_batch(Z, [0], [0.0], **kw)
    ctx.regrid_batch(Z, [capi.FIXED, capi.CONTINUOUS, capi.FREE], np.linspace(tl[:, 0], tl[:, -1], 3, axis=1), **kw)


def free_calls(ctx, X0, tf):
    """The entry points that read no shooting problem."""
    from socp_amd import capi
    ctx.integrate_batch(0.0, tf, X0)
    for what in (capi.EVAL_RHS, capi.EVAL_CONTROL, capi.EVAL_HAMILTONIAN):
        ctx.eval_batch(what, 0.5 * tf, X0)
    ctx.integrate_dense(0.0, tf, X0[0], cap=64)


def goddard(variant, integrator, mu2):
    from socp_amd import capi
    from conftest import goddard_c1_problem
    from test_gpu_cost_batch import build_goddard_c1
    ctx, o, _, Z, _ = build_goddard_c1(B=3, N=4, variant=variant)
    prob, _ = goddard_c1_problem(o)
    ctx.set_param("mu2", mu2)
    if integrator == capi.INT_DOPRI5:
        ctx.set_integrator(capi.INT_DOPRI5, 1e-6)
    fixed = integrator == capi.INT_RK4
    print("goddard %s integrator %d mu2 %g" % (variant, integrator, mu2), flush=True)
    free_calls(ctx, Z[:, :14], 0.01)
    problem_calls(ctx, Z, None, fixed=fixed)
    B = len(Z)
    time = np.tile(prob.time, (B, 1))
    xnode = np.tile(prob.xnode.ravel(), (B, 1))
    for smooth in (0, 1):
        params = np.tile(np.concatenate([ctx.get_params(), [0.0227, 0.08]]), (B, 1))
        if smooth:
            params[:, 6] = 1.0
        ctx._chk(ctx.L.socp_problem_blocks_all_smooth(ctx.h, smooth))
        problem_calls(ctx, Z, (params, time, xnode), fixed=fixed)
    ctx.close()


def other(build, name, tf):
    from socp_amd import capi
    for variant in ("exact", "fast"):
        ctx, _, _, Z, _ = build(B=3, N=4, variant=variant)
        print("%s %s" % (name, variant), flush=True)
        free_calls(ctx, Z[:, :ctx.s], tf)
        problem_calls(ctx, Z, None)
        if ctx.has_variational():
            ctx.var_jacobian(Z[0])
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--names", metavar="DIR", help="print the kernel names of the trace under DIR in launch order and exit")
    args = ap.parse_args()
    if args.names:
        return names(args.names)
    from socp_amd import capi
    from test_gpu_cost_batch import build_dint_wp, build_covid
    for variant in ("exact", "fast"):
        for integrator in (capi.INT_RK4, capi.INT_DOPRI5):
            for mu2 in (0.0, 1.0):
                goddard(variant, integrator, mu2)
    other(build_dint_wp, "double integrator", 1.0)
    other(build_covid, "covid19", 1.0)


if __name__ == "__main__":
    main()
