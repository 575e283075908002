#!/usr/bin/env python3
"""Batched branch following (socp_branch_batch_dev) against the same rounds composed from what the library offered before it:
residual rows with per-row blocks (socp_problem_set_blocks_dev + socp_residual_batch_dev), socp_fd_jacobian_multi_dev, torch tensor
operations for the bordered matrices and the per-row decisions, torch.linalg.solve.  Also one round against one
socp_tangent_batch_dev call with K = 1 on the same rows.  Writes one JSON object to profiles/branch_timing.json (--out PATH for
another place) and prints it.

    python tests/tools/branch_timing.py

Workload: Goddard, KD 310 -> 0 (wtheta 310), 4096 rows of the six-segment layout (n = 85) and 13 107 rows of single shooting
(n = 14), 100-step and 10^4-step trajectories, both flavours; every row starts from one Newton-polished root, --rounds rounds per
call (the _dev form: no early stop).  HIP events, warm-up first, the sides alternated in one process, median of 5, all five kept.
Bar: composed / call >= 1.0."""
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
ap.add_argument("--batch85", type=int, default=4096)
ap.add_argument("--steps", type=int, nargs="+", default=[100, 10000])
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "branch_timing.json"))
args = ap.parse_args()
KD, WTHETA, FTOL, H0, HMAX, MAXCORR, KFAST = 2, 310.0, 1e-10, 0.1, 0.4, 6, 2


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


def newton(ctx, z, iters=15):
    for _ in range(iters):
        F = ctx.residual(z)
        z = z + np.linalg.solve(ctx.fd_jacobian(z, F, dedup=True), -F)
    return z, float(np.max(np.abs(ctx.residual(z))))


def composed(ctx, B, n, dZ, rounds, cap):
    """The rounds of include/socp_hip.h ("Past a fold") with torch for everything the library did not offer before."""
    dev, f64 = "cuda", torch.float64
    n1, e = n + 1, float(np.sqrt(max(1e-15, np.finfo(np.float64).eps)))
    block = torch.tensor(np.concatenate([ctx.get_params()[:8], [0.0, 0.0]]), dtype=f64, device=dev)
    wP = block.repeat(2 * B, 1).contiguous()
    wZ = torch.empty(2 * B, n, dtype=f64, device=dev)
    wF = torch.empty(2 * B, n, dtype=f64, device=dev)
    wJ = torch.empty(B, n * n, dtype=f64, device=dev)
    v = torch.cat([dZ.view(B, n), torch.full((B, 1), float(block[KD]) / WTHETA, dtype=f64, device=dev)], dim=1)
    y, t = v.clone(), torch.zeros(B, n1, dtype=f64, device=dev)
    h = torch.full((B,), H0, dtype=f64, device=dev)
    k = torch.zeros(B, dtype=torch.int32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    count = torch.zeros(B, dtype=torch.int64, device=dev)
    Y = torch.full((B, cap, n1), float("nan"), dtype=f64, device=dev)
    rows = torch.arange(B, device=dev)
    unit = torch.zeros(B, n1, dtype=f64, device=dev)
    unit[:, n] = 1.0
    ctx._chk(ctx.L.socp_problem_set_blocks_dev(ctx.h, wP.data_ptr(), 10, None, None))
    try:
        for rnd in range(rounds):
            theta = v[:, n] * WTHETA
            hth = torch.where(theta == 0, torch.full_like(theta, e), e * theta.abs())
            wP[:B, KD], wP[B:, KD] = theta, theta + hth
            wZ[:B], wZ[B:] = v[:, :n], v[:, :n]
            ctx.residual_batch_dev(2 * B, wZ.data_ptr(), wF.data_ptr())
            ctx.fd_jacobian_multi_dev(B, wZ.data_ptr(), wF.data_ptr(), 1e-15, wJ.data_ptr(), dedup=True)
            F0, F1 = wF[:B], wF[B:]
            rn = F0.abs().max(dim=1).values
            M = torch.empty(B, n1, n1, dtype=f64, device=dev)
            M[:, :n, :n] = wJ.view(B, n, n).transpose(1, 2)
            M[:, :n, n] = (F1 - F0) / hth[:, None] * WTHETA
            M[:, n, :] = -unit if rnd == 0 else t
            live = status == 0
            accept = live & ((rn <= FTOL) | (rnd == 0))
            reject = live & ~accept & (~torch.isfinite(rn) | (k == MAXCORR))
            correct = live & ~accept & ~reject
            rhs = torch.where(correct[:, None], torch.cat([-F0, torch.zeros(B, 1, dtype=f64, device=dev)], dim=1), unit)
            x = torch.linalg.solve(M, rhs)
            norm = x.norm(dim=1)
            reject = reject | (correct & ~(norm <= h))
            correct = correct & ~reject
            v = torch.where(correct[:, None], v + x, v)
            k = torch.where(correct, k + 1, k)
            y = torch.where(accept[:, None], v, y)
            rec = torch.cat([v[:, :n], theta[:, None]], dim=1)
            slot = count.clamp(max=cap - 1)
            Y[rows, slot] = torch.where(accept[:, None], rec, Y[rows, slot])
            count = count + accept.to(torch.int64)
            t = torch.where(accept[:, None], x / norm[:, None], t)
            grow = accept & (k <= KFAST) & (rnd > 0)
            h = torch.where(grow, (h * 2.0).clamp(max=HMAX), h)
            h = torch.where(reject, h / 2.0, h)
            reached = accept & (theta <= 0.0)
            status = torch.where(reached, torch.ones_like(status), status)
            status = torch.where(accept & ~reached & (count >= cap), torch.full_like(status, 2), status)
            status = torch.where(reject & (h < 1e-8), torch.full_like(status, 3), status)
            predict = (accept | reject) & (status == 0)
            v = torch.where(predict[:, None], y + h[:, None] * t, v)
            k = torch.where(predict, torch.zeros_like(k), k)
    finally:
        ctx.L.socp_problem_set_blocks_dev(ctx.h, None, 0, None, None)
    return status, count


def shape(segments, B, steps):
    ctx = capi.Context(capi.MODEL_GODDARD)
    ctx.set_params(sweep.GODDARD_PARAMS)
    ctx.set_step_number(steps)
    Z = sweep.goddard_starts(1, 0.0)
    if segments == 1:
        sweep.goddard_single_shooting_problem(ctx)
    else:
        sweep.goddard_multiple_shooting_problem(ctx, segments)
        Z = sweep.goddard_multiple_shooting_starts(ctx, Z, segments)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    n, cap = ctx.n, 16
    z0, fnorm = newton(ctx, np.array(Z[0]))
    dZ = torch.from_numpy(np.ascontiguousarray(np.tile(z0, (B, 1)))).cuda()
    opts = capi.branch_options(wtheta=WTHETA, dir=-1, goal=0.0, h0=H0, hmax=HMAX, max_corr=MAXCORR, kfast=KFAST, ftol=FTOL, cap=cap, rounds=args.rounds)
    one = capi.branch_options(wtheta=WTHETA, dir=-1, goal=0.0, h0=H0, hmax=HMAX, max_corr=MAXCORR, kfast=KFAST, ftol=FTOL, cap=cap, rounds=1)
    wb, tb = ctx.branch_work_bytes(B), ctx.tangent_work_bytes(B, 1)
    work = torch.empty(max(wb, tb), dtype=torch.uint8, device="cuda")
    f = lambda *s: torch.empty(*s, dtype=torch.float64, device="cuda")  # noqa: E731
    i = lambda *s: torch.empty(*s, dtype=torch.int32, device="cuda")  # noqa: E731
    outs = [f(B * cap * (n + 1)), f(B * cap), f(B * cap), i(B), i(B), i(B), i(B), i(B), f(B), f(B * n)]
    dD, dI = f(B * n), i(B)
    out = {"n": n, "M": segments, "B": B, "step_nbr": steps, "rounds": args.rounds, "work_bytes": wb, "start_fnorm": fnorm}
    for variant in ("exact", "fast"):
        ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)

        def call(o=opts):
            ctx.branch_batch_dev(B, dZ.data_ptr(), (capi.DIR_PARAM, KD), o, work.data_ptr(), wb, *(a.data_ptr() for a in outs))
        kept = {}

        def compose():
            kept["status"], kept["count"] = composed(ctx, B, n, dZ, args.rounds, cap)
        (call_ms, comp_ms, round_ms, tan_ms), raw = median_ms(
            [call, compose, lambda: call(one),
             lambda: ctx.tangent_batch_dev(B, dZ.data_ptr(), [(capi.DIR_PARAM, KD)], 1e-15, 0, work.data_ptr(), tb, dD.data_ptr(), dI.data_ptr(), None)])
        call()
        torch.cuda.synchronize()
        ratio = comp_ms / call_ms
        out[variant] = {"branch_ms": call_ms, "composed_ms": comp_ms, "composed_over_branch": ratio, "bar_1.0": "met" if ratio >= 1.0 else "NOT met",
                        "one_round_ms": round_ms, "tangent_K1_ms": tan_ms, "round_over_tangent": round_ms / tan_ms,
                        "points_after_rounds": [int(outs[3].min().item()), int(outs[3].max().item())],
                        "composed_points_after_rounds": [int(kept["count"].min().item()), int(kept["count"].max().item())],
                        "status_histogram": np.bincount(outs[6].cpu().numpy(), minlength=6).tolist(),
                        "branch_ms_all": raw[0], "composed_ms_all": raw[1], "one_round_ms_all": raw[2], "tangent_K1_ms_all": raw[3]}
    ctx.close()
    return out


result = {"device": torch.cuda.get_device_name(0), "reps": 5}
for steps in args.steps:
    result["goddard_n85_N%d" % steps] = shape(6, args.batch85, steps)
    result["goddard_n14_N%d" % steps] = shape(1, args.batch14, steps)
    with open(args.out, "w") as fh:                                # kept after every shape: a later one may run long
        fh.write(json.dumps(result, indent=1) + "\n")
print(json.dumps(result, indent=1))
