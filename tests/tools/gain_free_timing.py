#!/usr/bin/env python3
"""Batched neighbouring-extremal gains with a FREE final time (socp_gain_free_batch_dev) on the GPU box beside socp_gain_batch_dev on
the fixed-time twin problem (the same rows, t_f FIXED at the shared value): what the length lane, the dual step and the bordered
sweep cost.  The project's precedent is the exact Jacobian at 1.01 - 1.02 x the all-columns fields call (15 lanes per group fill the
same four groups per wave as 14), so the aim is free / twin <= 1.10; the JSON says met or NOT met.
Writes one JSON object to profiles/gain_free_timing.json (--out PATH for another place) and prints it.

    python tests/tools/gain_free_timing.py

Workload: Goddard single shooting (M = 1, d = 7), B = 13 107, stride 100, at 100 and 10^4 RK4 steps, both flavours, both sides in one
process on device-resident rows.  HIP events, warm-up first, the sides alternated, median of 5 with the spread.  The aim is read at
mu2 = 1 (the smooth-law kernels); the same pair at mu2 = 0 (the general-law kernels, whose free-time blocks kernel has a private segment) is
reported beside it."""
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
ap.add_argument("--stride", type=int, default=100)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gain_free_timing.json"))
args = ap.parse_args()
B, D, S = args.batch, 7, 14
dev = "cuda"


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


def context(steps, variant, free_tf, law="smooth"):
    ctx = capi.Context(capi.MODEL_GODDARD)
    P = np.array(sweep.GODDARD_PARAMS, dtype=np.float64)
    if law == "general":                                              # mu2 = 0: bang-singular-off with the two switching times given
        P[6] = 0.0
    ctx.set_params(P)
    if law == "general":
        ctx.set_switching_times((0.05, 0.15))
    ctx.set_step_number(steps)
    if free_tf:
        assert sweep.goddard_multiple_shooting_problem(ctx, 1) == S + 1          # the testGoddard layout with one segment: t_f FREE
    else:
        sweep.goddard_single_shooting_problem(ctx)
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    return ctx


def one(steps, variant, law="smooth"):
    Q = max(1, -(-steps // args.stride))
    free, twin = context(steps, variant, True, law), context(steps, variant, False, law)
    f64 = dict(dtype=torch.float64, device=dev)
    z14 = sweep.goddard_starts(B, 1e-3)
    dZ = torch.from_numpy(z14).cuda()
    dZf = torch.from_numpy(np.hstack([z14, np.full((B, 1), sweep.TF)])).cuda()
    tq, kp, ke = torch.empty((B, 1, Q), **f64), torch.empty((B, 1, Q, D, D), **f64), torch.empty((B, 1, Q, D, D + 1), **f64)
    tq2 = torch.empty((B, 1, Q), **f64)
    info, info2 = (torch.zeros((B, 1, Q), dtype=torch.int32, device=dev) for _ in range(2))
    cnt, cnt2 = (torch.zeros((B, 1), dtype=torch.int32, device=dev) for _ in range(2))

    def call_free():
        free.gain_free_batch_dev(B, dZf.data_ptr(), args.stride, Q, tq2.data_ptr(), ke.data_ptr(), info2.data_ptr(), cnt2.data_ptr())

    def call_twin():
        twin.gain_batch_dev(B, dZ.data_ptr(), args.stride, Q, tq.data_ptr(), kp.data_ptr(), info.data_ptr(), cnt.data_ptr())

    (t_free, t_twin), raw = median_ms([call_free, call_twin])
    torch.cuda.synchronize()
    ratio = t_free / t_twin
    out = {"step_nbr": steps, "blocks_per_row": Q, "free_ms": t_free, "twin_ms": t_twin, "free_over_twin": ratio,
           "aim_free_over_twin_le_1.10": "met" if ratio <= 1.10 else "NOT met",
           "free_ms_all": raw[0], "twin_ms_all": raw[1], "free_spread_ms": max(raw[0]) - min(raw[0]), "twin_spread_ms": max(raw[1]) - min(raw[1]),
           "samples_equal_tq": bool(torch.equal(tq, tq2)), "solved_samples_free": int((info2 == 0).sum().item()),
           "solved_samples_twin": int((info == 0).sum().item()), "samples": int(info.numel()),
           "workspace_bytes_free": (B * Q * ((D + 1) * (D + 1) + S * S + S) + B * S) * 8}
    free.close()
    twin.close()
    return out


result = {"B": B, "M": 1, "d": D, "stride": args.stride, "device": torch.cuda.get_device_name(0), "reps": 5}
for steps in args.steps:
    for variant in ("exact", "fast"):
        result["N%d_%s" % (steps, variant)] = one(steps, variant)
# the general-law kernels (mu2 = 0), which profiles/gain_free_kernel_meta.txt shows with a private segment: reported beside the aim
for steps in args.steps:
    result["N%d_exact_general_law" % steps] = one(steps, "exact", "general")
text = json.dumps(result, indent=1)
with open(args.out, "w") as f:
    f.write(text + "\n")
print(text)
