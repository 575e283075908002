#!/usr/bin/env python3
"""Batched event location (socp_events_batch_dev) against the residual (socp_residual_batch_dev) on the GPU box; writes one JSON
object to profiles/events_timing.json (--out PATH for another place) and prints it.

    python tests/tools/events_timing.py

Workload: Goddard single shooting (n = 14, M = 1), 10^4 RK4 steps, B = 13 107, both flavours, the launches on the same context
and the same device-resident Z.  Two watches in both event runs: once at levels no trajectory reaches (no crossing: the cost of
watching alone -- a residual launch plus one channel evaluation per step), once at -2 mu2 u_max and 0 (the crossings of the
control law, each refined by two false-position steps and its state stored).  HIP events, warm-up first, the three sides alternated
in one process, median of 5.  No bar is set: the ratios are what is reported, with the number of events found."""
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
ap.add_argument("--steps", type=int, default=10000)
ap.add_argument("--refine", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "events_timing.json"))
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


B, cap, s = args.batch, 4, 14
p = sweep.GODDARD_PARAMS
dZ = torch.from_numpy(sweep.goddard_starts(B, 1e-3)).cuda()
dF = torch.empty(B * 14, dtype=torch.float64, device="cuda")
quiet = torch.from_numpy(np.tile([-1e30, 1e30], (B, 1))).cuda()
cross = torch.from_numpy(np.tile([-2.0 * p[6] * p[4], 0.0], (B, 1))).cuda()
dT = torch.full((B, 1, cap), float("nan"), dtype=torch.float64, device="cuda")
dI = torch.zeros((B, 1, cap), dtype=torch.int32, device="cuda")
dC = torch.zeros((B, 1), dtype=torch.int32, device="cuda")
dX = torch.empty((B, 1, cap, s), dtype=torch.float64, device="cuda")


def events(levels):
    ctx.events_batch_dev(B, dZ.data_ptr(), [0, 0], levels.data_ptr(), args.refine, cap, dT.data_ptr(), dI.data_ptr(), dC.data_ptr(), dX.data_ptr())


out = {"B": B, "M": 1, "step_nbr": args.steps, "refine": args.refine, "cap": cap, "device": torch.cuda.get_device_name(0), "reps": 5}
for variant in ("exact", "fast"):
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    (res_ms, quiet_ms, cross_ms), raw = median_ms([lambda: ctx.residual_batch_dev(B, dZ.data_ptr(), dF.data_ptr()),
                                                   lambda: events(quiet), lambda: events(cross)])
    events(quiet)
    torch.cuda.synchronize()
    n_quiet = int(dC.sum().item())
    events(cross)
    torch.cuda.synchronize()
    count, ident = dC.cpu().numpy(), dI.cpu().numpy()
    stored = np.arange(cap)[None, None, :] < np.minimum(count, cap)[:, :, None]
    out[variant] = {"residual_ms": res_ms, "events_no_crossing_ms": quiet_ms, "events_crossing_ms": cross_ms,
                    "ratio_no_crossing": quiet_ms / res_ms, "ratio_crossing": cross_ms / res_ms,
                    "residual_ms_all": raw[0], "events_no_crossing_ms_all": raw[1], "events_crossing_ms_all": raw[2],
                    "events_found_no_crossing": n_quiet, "events_found_crossing": int(count.sum()), "events_per_row_max": int(count.max()),
                    "events_by_id": {str(k): int(np.sum(ident[stored] == k)) for k in np.unique(ident[stored])}}
text = json.dumps(out, indent=1)
with open(args.out, "w") as f:
    f.write(text + "\n")
print(text)
