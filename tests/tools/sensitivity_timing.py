#!/usr/bin/env python3
"""Batched exact sensitivities (socp_sensitivity_batch_dev) timed beside the calls it is built on; writes one JSON object to
profiles/sensitivity_timing.json (--out PATH for another place) and prints it.

    python tests/tools/sensitivity_timing.py

Per shape and K (parameter directions C, b, KD, ... in block order): the call; the same call with K boundary-value directions, which
launch no direction lane (the difference is the direction launch); socp_exact_jacobian_batch_dev alone; socp_tangent_batch_dev with
jac = 0 on the same rows and directions.  No bar: nothing composed from the earlier calls gives an exact dF/dtheta of a parameter.
Reported: the direction launch's share of the call and its cost per dual trajectory relative to the exact Jacobian's.

Workload: Goddard single shooting (n = 14), 13 107 rows, 100-step and 10^4-step trajectories, reference-order context (the kernels
are one object for both flavours); every row is the root moved by 1e-7 (relative, its own draw).  HIP events, warm-up first, the
sides alternated in one process, median of 5, all five kept."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from socp_amd import capi, sweep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=13107)
ap.add_argument("--steps", type=int, nargs="+", default=[100, 10000])
ap.add_argument("--dirs", type=int, nargs="+", default=[1, 8])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sensitivity_timing.json"))
args = ap.parse_args()


def median_ms(fns, reps=5):
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b))
    return [float(np.median(t)) for t in times], times


def shape(B, steps):
    ctx = capi.Context(capi.MODEL_GODDARD)
    ctx.set_params(sweep.GODDARD_PARAMS)
    ctx.set_step_number(steps)
    sweep.goddard_single_shooting_problem(ctx)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    n, S = ctx.n, 14
    root = ctx.newton_batch(np.array(sweep.goddard_starts(1, 0.0)), jac=2, ftol=1e-300, rounds=30, trials=8)["z"][0]
    Z = root[None, :] * (1.0 + 1e-7 * np.random.default_rng(steps).uniform(-1.0, 1.0, size=(B, n)))
    dZ = torch.from_numpy(np.ascontiguousarray(Z)).cuda()
    f = lambda *s: torch.empty(*s, dtype=torch.float64, device="cuda")  # noqa: E731
    dJ, info = f(B * n * n), torch.empty(B, dtype=torch.int32, device="cuda")
    out = {"n": n, "B": B, "step_nbr": steps}
    jac_ms = None
    for K in args.dirs:
        pdirs = [(capi.DIR_PARAM, q) for q in range(K)]
        xdirs = [(capi.DIR_XNODE, q % 7) for q in range(K)]
        ws, wt = ctx.sensitivity_work_bytes(B, K), ctx.tangent_work_bytes(B, K)
        work = torch.empty(max(ws, wt), dtype=torch.uint8, device="cuda")
        dz, g = f(B * K * n), f(B * K * n)
        (call_ms, nolane_ms, jac_ms, tan_ms), raw = median_ms([
            lambda: ctx.sensitivity_batch_dev(B, dZ.data_ptr(), pdirs, work.data_ptr(), ws, dz.data_ptr(), info.data_ptr(), g.data_ptr()),
            lambda: ctx.sensitivity_batch_dev(B, dZ.data_ptr(), xdirs, work.data_ptr(), ws, dz.data_ptr(), info.data_ptr(), g.data_ptr()),
            lambda: ctx.exact_jacobian_batch_dev(B, dZ.data_ptr(), dJ.data_ptr(), None),
            lambda: ctx.tangent_batch_dev(B, dZ.data_ptr(), pdirs, 1e-15, 0, work.data_ptr(), wt, dz.data_ptr(), info.data_ptr(), g.data_ptr())])
        lane_ms = call_ms - nolane_ms
        out["K%d" % K] = {"call_ms": call_ms, "call_without_direction_lanes_ms": nolane_ms, "direction_launch_ms": lane_ms,
                          "direction_launch_share_of_call": lane_ms / call_ms, "exact_jacobian_ms": jac_ms, "tangent_fd_ms": tan_ms,
                          "call_over_exact_jacobian": call_ms / jac_ms, "call_over_tangent_fd": call_ms / tan_ms,
                          "dual_trajectory_cost_over_exact_jacobians": (lane_ms / (B * K)) / (jac_ms / (B * (S + 1))),
                          "work_bytes": ws, "call_ms_all": raw[0], "call_without_direction_lanes_ms_all": raw[1],
                          "exact_jacobian_ms_all": raw[2], "tangent_fd_ms_all": raw[3]}
    ctx.close()
    return out


result = {"device": torch.cuda.get_device_name(0), "reps": 5}
for steps in args.steps:
    result["goddard_n14_N%d" % steps] = shape(args.batch, steps)
    with open(args.out, "w") as fh:                                # kept after every shape: a later one may run long
        fh.write(json.dumps(result, indent=1) + "\n")
print(json.dumps(result, indent=1))
