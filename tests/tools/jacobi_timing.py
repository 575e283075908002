#!/usr/bin/env python3
"""Batched Jacobi fields (socp_jacobi_batch_dev) on the GPU box against (a) the same job composed from the entry points the
library had before -- socp_trace_batch_dev on B (d + 1) explicitly perturbed rows at the same stride, then the differences,
torch.linalg.det and the sign test as tensor operations -- and (b) a residual launch of B (d + 1) rows at the same step count;
(c) is (b) with stride = 1.  Writes one JSON object to profiles/jacobi_timing.json (--out PATH for another place) and prints it.

    python tests/tools/jacobi_timing.py

Workload: Goddard single shooting (n = 14, M = 1, d = 7), 10^4 RK4 steps, B = 13 107, stride 100, both flavours, all sides on the
same context and the same device-resident Z.  HIP events, warm-up first, the sides alternated in one process, median of 5.
The bar for (a): composed_ms / jacobi_ms >= 1.0.  (b) and (c) are reported without a bar.  At stride 1 the call stores the first
`--cap1` samples only (all are counted and take part in the sign test): 10^4 stored samples per row would be 2 GB."""
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
ap.add_argument("--skip", type=int, default=1)
ap.add_argument("--cap1", type=int, default=4)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jacobi_timing.json"))
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


B, D, G, W = args.batch, 7, 8, ctx.trace_width()
samples = args.steps // args.stride + (1 if args.steps % args.stride else 0)
cap = samples
rows_cap = samples + 1                                     # the trace keeps the start row too
eps = float(np.sqrt(np.finfo(np.float64).eps))
dev = "cuda"
dZ = torch.from_numpy(sweep.goddard_starts(B, 1e-3)).cuda()
tq = torch.empty((B, 1, cap), dtype=torch.float64, device=dev)
det = torch.empty((B, 1, cap), dtype=torch.float64, device=dev)
cnt = torch.zeros((B, 1), dtype=torch.int32, device=dev)
nch = torch.zeros((B, 1), dtype=torch.int32, device=dev)
tcj = torch.empty((B, 1), dtype=torch.float64, device=dev)
rows = torch.empty((B * G, 1, rows_cap, W), dtype=torch.float64, device=dev)
rcount = torch.zeros((B * G, 1), dtype=torch.int32, device=dev)
dF = torch.empty((B * G, 14), dtype=torch.float64, device=dev)
keep = {}


def perturbed():
    """Zp[B (d + 1)][14]: row b (d + 1) + c = column c of row b, and the steps h[B][d]."""
    p = dZ[:, D:]
    h = eps * p.abs()
    h = torch.where(h == 0, torch.full_like(h, eps), h)
    Zp = dZ.repeat_interleave(G, dim=0).view(B, G, 2 * D)
    idx = torch.arange(D, device=dev)
    Zp[:, idx + 1, D + idx] += h
    return Zp.view(B * G, 2 * D), h


def jacobi(stride, c):
    ctx.jacobi_batch_dev(B, dZ.data_ptr(), 0.0, stride, args.skip, c, tq.data_ptr(), det.data_ptr(), cnt.data_ptr(), nch.data_ptr(), tcj.data_ptr())


def composed():
    Zp, h = perturbed()
    ctx.trace_batch_dev(B * G, Zp.data_ptr(), args.stride, rows_cap, rows.data_ptr(), rcount.data_ptr())
    r = rows.view(B, G, rows_cap, W)[:, :, 1:]                          # the samples (row 0 is the start)
    X = r[:, :, :, 1:1 + D]                                             # [B][c][sample][r]
    J = ((X[:, 1:] - X[:, :1]) / h[:, :, None, None]).permute(0, 2, 3, 1)      # [B][sample][r][c]
    d = torch.linalg.det(J)
    t = r[:, 0, :, 0]
    neg = d < 0
    ok = ~(torch.isnan(d[:, 1:]) | torch.isnan(d[:, :-1]))
    change = (neg[:, 1:] != neg[:, :-1]) & ok
    change[:, :args.skip] = False
    n = change.sum(dim=1)
    first = torch.argmax(change.to(torch.int8), dim=1, keepdim=True)
    d0, d1 = torch.gather(d, 1, first), torch.gather(d, 1, first + 1)
    t0, t1 = torch.gather(t, 1, first), torch.gather(t, 1, first + 1)
    tc = torch.where(n[:, None] > 0, t0 + (t1 - t0) * (d0 / (d0 - d1)), torch.full_like(t0, float("nan")))
    keep["composed"] = (d, n, tc)


def residual():
    Zp, _h = perturbed()
    ctx.residual_batch_dev(B * G, Zp.data_ptr(), dF.data_ptr())


out = {"B": B, "M": 1, "d": D, "step_nbr": args.steps, "stride": args.stride, "skip": args.skip, "samples_per_row": samples,
       "cap_at_stride_1": args.cap1, "device": torch.cuda.get_device_name(0), "reps": 5}
for variant in ("exact", "fast"):
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    (jac_ms, comp_ms, res_ms, jac1_ms), raw = median_ms([lambda: jacobi(args.stride, cap), composed, residual, lambda: jacobi(1, args.cap1)])
    jacobi(args.stride, cap)
    composed()
    torch.cuda.synchronize()
    d, n, _tc = keep["composed"]
    mine = det[:, 0]
    scale = mine.abs().amax(dim=1, keepdim=True)
    out[variant] = {"jacobi_ms": jac_ms, "composed_ms": comp_ms, "residual_ms": res_ms, "jacobi_stride1_ms": jac1_ms,
                    "ratio_a_composed_over_jacobi": comp_ms / jac_ms, "ratio_b_jacobi_over_residual": jac_ms / res_ms,
                    "ratio_c_jacobi_stride1_over_residual": jac1_ms / res_ms,
                    "jacobi_ms_all": raw[0], "composed_ms_all": raw[1], "residual_ms_all": raw[2], "jacobi_stride1_ms_all": raw[3],
                    "rows_with_change": int((nch[:, 0] > 0).sum().item()), "rows_with_change_composed": int((n > 0).sum().item()),
                    "max_det_difference_to_composed_rel_row_max": float(((mine - d).abs() / scale).max().item())}
text = json.dumps(out, indent=1)
with open(args.out, "w") as f:
    f.write(text + "\n")
print(text)
