#!/usr/bin/env python3
"""Batched running cost (socp_cost_batch_dev) against the residual (socp_residual_batch_dev) on the GPU box; writes one JSON
object to profiles/cost_timing.json (--out PATH for another place) and prints it.

    python tests/tools/cost_timing.py

Workload: the bench shape -- Goddard single shooting (n = 14, M = 1), 10^4 RK4 steps, B = 196 605 (the bench headline's
trajectory count) -- both flavours, the two launches on the same context and the same device-resident Z.  HIP events, warm-up
first, the two sides alternated in one process, median of 5.  No bar is set: the ratio is what is reported.  The cost kernel
evaluates the Hamiltonian beside the right-hand side at each of the four stages of a step, and stores cost and total only."""
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
ap.add_argument("--batch", type=int, default=196605)
ap.add_argument("--steps", type=int, default=10000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cost_timing.json"))
args = ap.parse_args()

ctx = capi.Context(capi.MODEL_GODDARD)
ctx.set_params(sweep.GODDARD_PARAMS)
ctx.set_step_number(args.steps)
sweep.goddard_single_shooting_problem(ctx)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)


def median_ms(fns, reps=5):
    """Median of `reps` event-timed calls of every function, the functions alternated inside each repetition."""
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


B = args.batch
dZ = torch.from_numpy(sweep.goddard_starts(B, 1e-3)).cuda()
dF = torch.empty(B * 14, dtype=torch.float64, device="cuda")
dC = torch.empty(B, dtype=torch.float64, device="cuda")
dT = torch.empty(B, dtype=torch.float64, device="cuda")
out = {"B": B, "M": 1, "step_nbr": args.steps, "device": torch.cuda.get_device_name(0), "reps": 5}
costs = {}
for variant in ("exact", "fast"):
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    (res_ms, cost_ms), raw = median_ms([lambda: ctx.residual_batch_dev(B, dZ.data_ptr(), dF.data_ptr()),
                                        lambda: ctx.cost_batch_dev(B, dZ.data_ptr(), dC.data_ptr(), dT.data_ptr(), None)])
    costs[variant] = dC.cpu().numpy()
    out[variant] = {"residual_ms": res_ms, "cost_ms": cost_ms, "ratio": cost_ms / res_ms, "residual_ms_all": raw[0], "cost_ms_all": raw[1],
                    "cost_min": float(costs[variant].min()), "cost_max": float(costs[variant].max())}
out["fast_vs_exact_max_abs_cost_deviation"] = float(np.max(np.abs(costs["fast"] - costs["exact"])))
text = json.dumps(out, indent=1)
with open(args.out, "w") as f:
    f.write(text + "\n")
print(text)
