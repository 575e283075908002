#!/usr/bin/env python3
"""Batched exact fields (socp_fields_batch_dev) on the GPU box beside (a) socp_jacobi_batch_dev -- the forward-difference instrument,
d + 1 trajectories per row -- on the same rows, in both flavours, and (b) a residual launch of B M C rows at the same step count.
No bars: this is a capability, and no composition of the library's earlier entry points gives the exact fields of Goddard.
Writes one JSON object to profiles/fields_timing.json (--out PATH for another place) and prints it.

    python tests/tools/fields_timing.py

Workload: Goddard single shooting (n = 14, M = 1, d = 7), 10^4 RK4 steps, B = 13 107, stride 100, both cols, all sides on the same
context and the same device-resident Z.  HIP events, warm-up first, the sides alternated in one process, median of 5.  The fields
kernels are one object for both flavours: a flavour changes only the jacobi and residual sides."""
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
ap.add_argument("--stride", type=int, default=100)
ap.add_argument("--skip", type=int, default=0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fields_timing.json"))
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


B, D = args.batch, 7
cap = args.steps // args.stride + (1 if args.steps % args.stride else 0)
dev = "cuda"
dZ = torch.from_numpy(sweep.goddard_starts(B, 1e-3)).cuda()
tq = torch.empty((B, 1, cap), dtype=torch.float64, device=dev)
det = torch.empty((B, 1, cap), dtype=torch.float64, device=dev)
cnt = torch.zeros((B, 1), dtype=torch.int32, device=dev)
nch = torch.zeros((B, 1), dtype=torch.int32, device=dev)
tcj = torch.empty((B, 1), dtype=torch.float64, device=dev)
phi = torch.empty((B, 1, 2 * D, 2 * D), dtype=torch.float64, device=dev)
rows = {C: dZ.repeat_interleave(C, dim=0).contiguous() for C in (D, 2 * D)}
dF = torch.empty((B * 2 * D, 14), dtype=torch.float64, device=dev)


def fields(cols):
    ctx.fields_batch_dev(B, dZ.data_ptr(), cols, args.stride, args.skip, cap, tq.data_ptr(), det.data_ptr(), cnt.data_ptr(), nch.data_ptr(),
                         tcj.data_ptr(), phi.data_ptr())


def jacobi():
    ctx.jacobi_batch_dev(B, dZ.data_ptr(), 0.0, args.stride, max(args.skip, 1), cap, tq.data_ptr(), det.data_ptr(), cnt.data_ptr(), nch.data_ptr(),
                         tcj.data_ptr())


def residual(C):
    ctx.residual_batch_dev(B * C, rows[C].data_ptr(), dF.data_ptr())


out = {"B": B, "M": 1, "d": D, "step_nbr": args.steps, "stride": args.stride, "skip": args.skip, "samples_per_row": cap,
       "device": torch.cuda.get_device_name(0), "reps": 5}
for variant in ("exact", "fast"):
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    (f0, f1, jac, r7, r14), raw = median_ms([lambda: fields(capi.FIELDS_COSTATE), lambda: fields(capi.FIELDS_ALL), jacobi,
                                             lambda: residual(D), lambda: residual(2 * D)])
    fields(capi.FIELDS_COSTATE)
    torch.cuda.synchronize()
    out[variant] = {"fields_costate_ms": f0, "fields_all_ms": f1, "jacobi_ms": jac, "residual_B_M_d_rows_ms": r7, "residual_B_M_2d_rows_ms": r14,
                    "fields_costate_over_jacobi": f0 / jac, "fields_all_over_jacobi": f1 / jac,
                    "fields_costate_over_residual": f0 / r7, "fields_all_over_residual": f1 / r14,
                    "fields_costate_ms_all": raw[0], "fields_all_ms_all": raw[1], "jacobi_ms_all": raw[2],
                    "residual_d_ms_all": raw[3], "residual_2d_ms_all": raw[4], "rows_with_change": int((nch[:, 0] > 0).sum().item())}
text = json.dumps(out, indent=1)
with open(args.out, "w") as f:
    f.write(text + "\n")
print(text)
