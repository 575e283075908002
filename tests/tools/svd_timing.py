#!/usr/bin/env python3
"""Batched singular values (socp_svd_batch_dev, Vt requested) against torch.linalg.svd on the same device tensor, and the share of
the decomposition in a whole socp_singular_batch_dev call; writes one JSON object to profiles/svd_timing.json (--out PATH for
another place) and prints it.

    python tests/tools/svd_timing.py

Two shapes, both flavours: the Jacobians of converged Goddard rows, single shooting (n = 14, B = 13 107) and the six-segment
layout (n = 85, B = 4096).  The rows are solved first (socp_chains_solve at 100 RK4 steps; a start that does not converge is
replaced by a converged one, cyclically), their forward-difference Jacobians taken at 100 steps.  HIP events, warm-up first, the
sides alternated in one process, median of 5 with the spread (min, max).  The parent commit has no equivalent, so the PyTorch
composition is the baseline; the goal is ratio = torch_ms / svd_ms >= 1.0, reported as met or not met per size and flavour.  When
one torch.linalg.svd call takes more than --torch-slow seconds it is timed once instead of five times (recorded as torch_reps).
The share of the decomposition in socp_singular_batch_dev (scale = 1) is taken at 10^4 and at 100 steps."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from socp_amd import capi, sweep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch14", type=int, default=13107)
ap.add_argument("--batch85", type=int, default=4096)
ap.add_argument("--steps-long", type=int, default=10000)
ap.add_argument("--steps-short", type=int, default=100)
ap.add_argument("--max-sweeps", type=int, default=60)
ap.add_argument("--torch-slow", type=float, default=5.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svd_timing.json"))
args = ap.parse_args()


def timed_ms(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def stats(times):
    return {"median_ms": float(np.median(times)), "min_ms": float(min(times)), "max_ms": float(max(times)), "all_ms": [float(t) for t in times]}


def alternated(fns, reps=5):
    """reps event-timed calls of every function, alternated inside each repetition, after one untimed call of each."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            times[k] += timed_ms(fn, 1)
    return [stats(t) for t in times]


def converged_rows(ctx, Z0):
    r = ctx.chains_solve(Z0, kind=capi.CHAIN_PLAIN, xtol=1e-8)
    good = np.nonzero(np.asarray(r["info"]) == 1)[0]
    if len(good) == 0:
        raise SystemExit("svd_timing: no start converged")
    Z = np.asarray(r["z"])[good[np.arange(len(Z0)) % len(good)]]
    return np.ascontiguousarray(Z), int(len(good))


def shape(segments, B):
    ctx = capi.Context(capi.MODEL_GODDARD)
    ctx.set_params(sweep.GODDARD_PARAMS)
    ctx.set_step_number(args.steps_short)
    Z0 = sweep.goddard_starts(B, 1e-3 if segments == 1 else 0.05)
    if segments == 1:
        sweep.goddard_single_shooting_problem(ctx)
    else:
        sweep.goddard_multiple_shooting_problem(ctx, segments)
        Z0 = sweep.goddard_multiple_shooting_starts(ctx, Z0, segments)
    Z, n_conv = converged_rows(ctx, Z0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    n = ctx.n
    dZ = torch.from_numpy(Z).cuda()
    dF = torch.empty(B * n, dtype=torch.float64, device="cuda")
    dJ = torch.empty((B, n, n), dtype=torch.float64, device="cuda")
    dS = torch.empty(B * n, dtype=torch.float64, device="cuda")
    dV = torch.empty(B * n * n, dtype=torch.float64, device="cuda")
    dv = torch.empty(B * n, dtype=torch.float64, device="cuda")
    dC = torch.empty(B * n, dtype=torch.float64, device="cuda")
    dW = torch.empty(B, dtype=torch.int32, device="cuda")
    dI = torch.empty(B, dtype=torch.int32, device="cuda")
    wb = ctx.singular_work_bytes(B)
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    out = {"n": n, "M": segments, "B": B, "rows_converged": n_conv, "max_sweeps": args.max_sweeps}

    def torch_svd():
        return torch.linalg.svd(dJ)
    for variant in ("exact", "fast"):
        ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
        ctx.set_step_number(args.steps_short)
        ctx.residual_batch_dev(B, dZ.data_ptr(), dF.data_ptr())
        ctx.fd_jacobian_multi_dev(B, dZ.data_ptr(), dF.data_ptr(), 1e-15, dJ.data_ptr(), dedup=True)
        torch.cuda.synchronize()

        def ours():
            ctx.svd_batch_dev(B, n, dJ.data_ptr(), args.max_sweeps, dS.data_ptr(), dV.data_ptr(), dW.data_ptr(), dI.data_ptr())
        t0 = time.perf_counter()
        torch_svd()
        torch.cuda.synchronize()
        first = time.perf_counter() - t0
        if first > args.torch_slow:                               # one more call is the measurement; the first was the warm-up
            mine = alternated([ours])[0]
            theirs = stats(timed_ms(torch_svd, 1))
            torch_reps = 1
        else:
            mine, theirs = alternated([ours, torch_svd])
            torch_reps = 5
        ours()
        torch.cuda.synchronize()
        # both sides against LAPACK on the host (numpy.linalg.svd), in units of n eps sigma_max
        lapack = np.linalg.svd(dJ.cpu().numpy(), compute_uv=False)
        unit = n * np.finfo(np.float64).eps * lapack[:, 0]
        dev = float(np.max(np.max(np.abs(dS.view(B, n).cpu().numpy() - lapack), axis=1) / unit))
        dev_torch = float(np.max(np.max(np.abs(torch_svd()[1].cpu().numpy() - lapack), axis=1) / unit)) if torch_reps == 5 else None
        ratio = theirs["median_ms"] / mine["median_ms"]
        rec = {"svd_batch": mine, "torch_linalg_svd": theirs, "torch_reps": torch_reps, "ratio_torch_over_svd_batch": ratio,
               "goal_ratio_ge_1": "met" if ratio >= 1.0 else "not met", "sweeps_max": int(dW.max().item()),
               "sweeps_median": float(dW.double().median().item()), "info_nonzero": int((dI != 0).sum().item()),
               "max_sigma_deviation_from_lapack_over_n_eps_sigma_max": dev,
               "torch_max_sigma_deviation_from_lapack_over_n_eps_sigma_max": dev_torch, "share": {}}
        for steps in (args.steps_long, args.steps_short):
            ctx.set_step_number(steps)

            def whole():
                ctx.singular_batch_dev(B, dZ.data_ptr(), 1e-15, 0, 1, args.max_sweeps, work.data_ptr(), wb, dS.data_ptr(), dv.data_ptr(),
                                       dC.data_ptr(), dW.data_ptr(), dI.data_ptr())
            whole()
            torch.cuda.synchronize()
            ctx.residual_batch_dev(B, dZ.data_ptr(), dF.data_ptr())
            ctx.fd_jacobian_multi_dev(B, dZ.data_ptr(), dF.data_ptr(), 1e-15, dJ.data_ptr(), dedup=True)
            torch.cuda.synchronize()
            scaled = (dJ / dJ.norm(dim=2, keepdim=True).clamp_min(1e-300)).contiguous()      # memory is [column][row]: unit columns

            def part():
                ctx.svd_batch_dev(B, n, scaled.data_ptr(), args.max_sweeps, dS.data_ptr(), None, dW.data_ptr(), dI.data_ptr())
            w, p = alternated([whole, part])
            rec["share"]["steps_%d" % steps] = {"singular_batch_dev": w, "decomposition": p, "share": p["median_ms"] / w["median_ms"]}
        out[variant] = rec
    ctx.close()
    return out


result = {"device": torch.cuda.get_device_name(0), "reps": 5, "goddard_n14": shape(1, args.batch14), "goddard_n85": shape(6, args.batch85)}
text = json.dumps(result, indent=1)
with open(args.out, "w") as f:
    f.write(text + "\n")
print(text)
