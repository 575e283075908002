#!/usr/bin/env python3
"""Batched tangent (socp_tangent_batch_dev) against the forward-difference Jacobian alone (socp_fd_jacobian_multi_dev) on the same
rows, and the share of the elimination (socp_linsolve_batch_dev on the call's own J and right-hand sides); writes one JSON object to
profiles/tangent_timing.json (--out PATH for another place) and prints it.

    python tests/tools/tangent_timing.py

Two shapes, both flavours: Goddard single shooting (M = 1, n = 14), 10^4 RK4 steps, B = 13 107, K = 1 (KD); the six-segment
layout (n = 85), B = 4096, K = 2 (KD, C).  HIP events, warm-up first, the three sides alternated in one process, median of 5.  No
bar is set: the expectation from the operation counts is that the trajectories dominate and the solve is a few percent."""
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
ap.add_argument("--batch14", type=int, default=13107)
ap.add_argument("--steps14", type=int, default=10000)
ap.add_argument("--batch85", type=int, default=4096)
ap.add_argument("--steps85", type=int, default=100)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tangent_timing.json"))
args = ap.parse_args()


def median_ms(fns, before, reps=5):
    """Median of `reps` event-timed calls of every function, alternated inside each repetition; before[k]() runs untimed first."""
    for pre, fn in zip(before, fns):
        pre()
        fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            before[k]()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b))
    return [float(np.median(t)) for t in times], times


def shape(segments, B, steps, dirs):
    ctx = capi.Context(capi.MODEL_GODDARD)
    ctx.set_params(sweep.GODDARD_PARAMS)
    ctx.set_step_number(steps)
    Z = sweep.goddard_starts(B, 1e-3)
    if segments == 1:
        sweep.goddard_single_shooting_problem(ctx)
    else:
        sweep.goddard_multiple_shooting_problem(ctx, segments)
        Z = sweep.goddard_multiple_shooting_starts(ctx, Z, segments)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    n, K = ctx.n, len(dirs)
    dZ = torch.from_numpy(np.ascontiguousarray(Z)).cuda()
    dF = torch.empty(B * n, dtype=torch.float64, device="cuda")
    dJ = torch.empty(B * n * n, dtype=torch.float64, device="cuda")
    dD = torch.empty(B * K * n, dtype=torch.float64, device="cuda")
    dG = torch.empty(B * K * n, dtype=torch.float64, device="cuda")
    dY = torch.empty(B * K * n, dtype=torch.float64, device="cuda")
    dI = torch.empty(B, dtype=torch.int32, device="cuda")
    wb = ctx.tangent_work_bytes(B, K)
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    out = {"n": n, "M": segments, "B": B, "K": K, "step_nbr": steps, "work_bytes": wb}
    for variant in ("exact", "fast"):
        ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
        ctx.residual_batch_dev(B, dZ.data_ptr(), dF.data_ptr())
        ctx.fd_jacobian_multi_dev(B, dZ.data_ptr(), dF.data_ptr(), 1e-15, dJ.data_ptr(), dedup=True)

        def tangent():
            ctx.tangent_batch_dev(B, dZ.data_ptr(), dirs, 1e-15, 0, work.data_ptr(), wb, dD.data_ptr(), dI.data_ptr(), dG.data_ptr())
        tangent()
        torch.cuda.synchronize()
        (tan_ms, jac_ms, lin_ms), raw = median_ms(
            [tangent,
             lambda: ctx.fd_jacobian_multi_dev(B, dZ.data_ptr(), dF.data_ptr(), 1e-15, dJ.data_ptr(), dedup=True),
             lambda: ctx.linsolve_batch_dev(B, n, K, dJ.data_ptr(), dY.data_ptr(), dI.data_ptr())],
            [lambda: None, lambda: None, lambda: dY.copy_(-dG)])             # (the matrix fits LDS at both shapes: J is left as it was)
        tangent()
        torch.cuda.synchronize()
        out[variant] = {"tangent_ms": tan_ms, "fd_jacobian_ms": jac_ms, "linsolve_ms": lin_ms, "tangent_over_jacobian": tan_ms / jac_ms,
                        "linsolve_share": lin_ms / tan_ms, "info_nonzero": int((dI != 0).sum().item()),
                        "tangent_ms_all": raw[0], "fd_jacobian_ms_all": raw[1], "linsolve_ms_all": raw[2]}
    ctx.close()
    return out


result = {"device": torch.cuda.get_device_name(0), "reps": 5,
          "goddard_n14": shape(1, args.batch14, args.steps14, [(capi.DIR_PARAM, 2)]),
          "goddard_n85": shape(6, args.batch85, args.steps85, [(capi.DIR_PARAM, 2), (capi.DIR_PARAM, 0)])}
text = json.dumps(result, indent=1)
with open(args.out, "w") as f:
    f.write(text + "\n")
print(text)
