#!/usr/bin/env python3
"""Batched exact shooting Jacobian (socp_exact_jacobian_batch_dev) on the GPU box beside (a) socp_fd_jacobian_multi_dev -- the forward
difference every other consumer reads -- on the same rows, and (b) socp_fields_batch_dev(SOCP_FIELDS_ALL), which produces S of its
S + 1 columns, in both flavours, at 10^4 and at 100 RK4 steps.  No bars: no composition of the library's earlier entry points gives
this matrix.  Writes one JSON object to profiles/exact_jacobian_timing.json (--out PATH for another place) and prints it.

    python tests/tools/exact_jacobian_timing.py

Workload: Goddard single shooting (n = 14, M = 1, d = 7), B = 13 107, all sides on the same context and the same device-resident Z
(the forward difference at (z, F(z)) with F from socp_residual_batch_dev of the context's own flavour, in a buffer the exact call
does not write; epsfcn 1e-15).  HIP events, warm-up first, the sides alternated in
one process, median of 5.  The exact-Jacobian and fields kernels are one object for both flavours: a flavour changes only the
forward-difference side."""
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
ap.add_argument("--steps", type=int, nargs="+", default=[10000, 100])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_jacobian_timing.json"))
args = ap.parse_args()

ctx = capi.Context(capi.MODEL_GODDARD)
ctx.set_params(sweep.GODDARD_PARAMS)
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


B, D, n = args.batch, 7, 14
dev = "cuda"
dZ = torch.from_numpy(sweep.goddard_starts(B, 1e-3)).cuda()
dJ = torch.empty((B, n * n), dtype=torch.float64, device=dev)
dJfd = torch.empty((B, n * n), dtype=torch.float64, device=dev)
dF = torch.empty((B, n), dtype=torch.float64, device=dev)          # the exact call's F: the reference-order residual
dFfd = torch.empty((B, n), dtype=torch.float64, device=dev)        # the forward difference's F: the context's own flavour
tq = torch.empty((B, 1, 1), dtype=torch.float64, device=dev)
det = torch.empty((B, 1, 1), dtype=torch.float64, device=dev)
cnt = torch.zeros((B, 1), dtype=torch.int32, device=dev)
nch = torch.zeros((B, 1), dtype=torch.int32, device=dev)
tcj = torch.empty((B, 1), dtype=torch.float64, device=dev)
phi = torch.empty((B, 1, n, n), dtype=torch.float64, device=dev)

out = {"B": B, "M": 1, "d": D, "n": n, "device": torch.cuda.get_device_name(0), "reps": 5, "runs": []}
for steps in args.steps:
    ctx.set_step_number(steps)

    def exact():
        ctx.exact_jacobian_batch_dev(B, dZ.data_ptr(), dJ.data_ptr(), dF.data_ptr())

    def fd():
        ctx.fd_jacobian_multi_dev(B, dZ.data_ptr(), dFfd.data_ptr(), 1e-15, dJfd.data_ptr())

    def fields():
        ctx.fields_batch_dev(B, dZ.data_ptr(), capi.FIELDS_ALL, steps, 0, 1, tq.data_ptr(), det.data_ptr(), cnt.data_ptr(), nch.data_ptr(),
                             tcj.data_ptr(), phi.data_ptr())

    for variant in ("exact", "fast"):
        ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
        ctx.residual_batch_dev(B, dZ.data_ptr(), dFfd.data_ptr())
        (e, f, p), raw = median_ms([exact, fd, fields])
        torch.cuda.synchronize()
        big = dJ.abs().amax(dim=1)
        dev_fd = ((dJfd - dJ).abs().amax(dim=1) / big)
        out["runs"].append({"step_nbr": steps, "variant": variant, "exact_jacobian_ms": e, "fd_jacobian_ms": f, "fields_all_ms": p,
                            "exact_over_fd": e / f, "exact_over_fields_all": e / p, "exact_jacobian_ms_all": raw[0], "fd_jacobian_ms_all": raw[1],
                            "fields_all_ms_all": raw[2], "fd_dev_median": float(dev_fd.nanmedian().item()),
                            "rows_finite": int(torch.isfinite(dJ).all(dim=1).sum().item())})
text = json.dumps(out, indent=1)
with open(args.out, "w") as f:
    f.write(text + "\n")
print(text)
