#!/usr/bin/env python3
"""Closed-loop flight under the sampled neighbouring-extremal law (socp_guide_batch_dev) on the GPU box:
(a) the call against the same job COMPOSED from existing calls -- one socp_integrate_batch_dev launch per sample block (a context
    whose step number is the stride, per-lane t0 / tf), the correction and, with a free final time, the re-timing as torch tensor
    operations, the host driving the loop.  The aim is composed / call >= 1.0; the JSON says met or NOT met;
(b) the call against ONE socp_residual_batch_dev launch of the same B K M trajectories in the same flavour -- recorded, no bar;
(c) every = 0 against every = 1: what the law itself costs.
Writes one JSON object to profiles/guide_timing.json (--out PATH for another place) and prints it.

    python tests/tools/guide_timing.py

Workload: Goddard (M = 1, d = 7, mu2 = 1), B = 13 107 rows, K = 15 cases (196 605 lanes), stride 100, every = 1, at 100 and 10^4 RK4
steps, both flavours, fixed and free final time, everything in one process on device-resident data.  HIP events, warm-up first, the
sides alternated, three warm-up rounds, median of 5 with the spread.  The composed side does what the call does up to the clamped last step of a segment
(each of its blocks ends on its own tf): it is a timing twin, its results are compared with the call's only loosely, and at 100 steps only."""
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
ap.add_argument("--cases", type=int, default=15)
ap.add_argument("--steps", type=int, nargs="+", default=[100, 10000])
ap.add_argument("--stride", type=int, default=100)
ap.add_argument("--sigma", type=float, default=1e-6)
ap.add_argument("--variants", nargs="+", default=["exact", "fast"], choices=["exact", "fast"])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guide_timing.json"))
args = ap.parse_args()
B, K, D, S = args.batch, args.cases, 7, 14
dev = "cuda"


def median_ms(fns, reps=5, warm=3):
    """Median of `reps` event-timed calls of every function, the functions alternated inside each repetition, after `warm` untimed
    rounds of all of them (one is too few for the clocks to settle: the first timed series fell monotonically)."""
    for _ in range(warm):
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


def context(steps, variant, free_tf):
    ctx = capi.Context(capi.MODEL_GODDARD)
    ctx.set_params(np.array(sweep.GODDARD_PARAMS, dtype=np.float64))
    ctx.set_step_number(steps)
    if free_tf:
        assert sweep.goddard_multiple_shooting_problem(ctx, 1) == S + 1          # the testGoddard layout with one segment: t_f FREE
    else:
        sweep.goddard_single_shooting_problem(ctx)
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    return ctx


def one(steps, variant, free_tf):
    Q = max(1, -(-steps // args.stride))
    ctx, block = context(steps, variant, free_tf), context(args.stride, variant, free_tf)
    f64 = dict(dtype=torch.float64, device=dev)
    z14 = sweep.goddard_starts(B, 1e-3)
    Z = torch.from_numpy(np.hstack([z14, np.full((B, 1), sweep.TF)]) if free_tf else z14).cuda()
    tables = (ctx.gain_free_batch if free_tf else ctx.gain_batch)(Z, stride=args.stride, xq=True)
    kg, xq, info, count = tables["ke" if free_tf else "kp"].contiguous(), tables["xq"], tables["info"], tables["count"]
    rng = np.random.default_rng(1)
    dX0 = torch.from_numpy(args.sigma * np.maximum(1.0, np.abs(z14[:, None, :D])) * rng.standard_normal((B, K, D))).cuda()
    NM = D + 1 if free_tf else D
    xf, miss = torch.empty((B, K, S), **f64), torch.empty((B, K, NM), **f64)
    nupd, nskip = (torch.zeros((B, K), dtype=torch.int32, device=dev) for _ in range(2))

    def call(every):
        ctx.guide_batch_dev(B, Z.data_ptr(), args.stride, Q, xq.data_ptr(), kg.data_ptr(), info.data_ptr(), count.data_ptr(), K, dX0.data_ptr(),
                            every, xf.data_ptr(), miss.data_ptr(), nupd.data_ptr(), nskip.data_ptr())

    # (a) the composed twin: lanes [B K], one integrate launch per block, the law in tensor operations
    X, X2 = torch.empty((B * K, S), **f64), torch.empty((B * K, S), **f64)
    t0, t1 = torch.empty(B * K, **f64), torch.empty(B * K, **f64)
    tf_nom = Z[:, -1] if free_tf else torch.full((B,), sweep.TF, **f64)
    ok = (info[:, 0] == 0)                                                      # [B][Q]

    def composed():
        nonlocal X, X2
        X[:, :D] = (Z[:, None, :D] + dX0).reshape(B * K, D)
        X[:, D:] = Z[:, None, D:S].expand(B, K, D).reshape(B * K, D)
        tf = tf_nom[:, None].expand(B, K).reshape(B * K).clone()
        for q in range(Q):
            dx = X[:, :D].reshape(B, K, D) - xq[:, 0, q, None, :D]
            corr = torch.einsum("bcr,bkc->bkr", kg[:, 0, q], dx)               # kg[b][c][r] = d(p_r, t_f)/dx_c
            p = xq[:, 0, q, None, D:] + corr[..., :D]
            m = ok[:, q, None, None]
            X[:, D:] = torch.where(m, p, X[:, D:].reshape(B, K, D)).reshape(B * K, D)
            if free_tf:
                tf = torch.where(ok[:, q, None], tf_nom[:, None] + corr[..., D], tf.reshape(B, K)).reshape(B * K)
            dt = tf / steps
            torch.mul(dt, float(q * args.stride), out=t0)
            torch.clamp(dt * float(min((q + 1) * args.stride, steps)), max=tf, out=t1)
            block.set_step_number(min(args.stride, steps - q * args.stride))
            block.integrate_batch_dev(B * K, t0.data_ptr(), t1.data_ptr(), None, X.data_ptr(), X2.data_ptr())
            X, X2 = X2, X
        return X

    # (b) one residual launch of the same number of trajectories
    Zr = Z[:, None, :].expand(B, K, Z.shape[1]).reshape(B * K, Z.shape[1]).contiguous()
    Fr = torch.empty_like(Zr)

    def residual():
        ctx.residual_batch_dev(B * K, Zr.data_ptr(), Fr.data_ptr())

    (t_call, t_comp, t_res, t_open), raw = median_ms([lambda: call(1), composed, residual, lambda: call(0)])
    call(1)
    torch.cuda.synchronize()
    twin = composed()[:, :S].reshape(B, K, S)
    # the twin's results beside the call's: read at 100 steps only -- the starts are unconverged, and over 10^4 steps the two
    # roundings of such a flight part by many orders, which says nothing about the twin doing the same job
    finite = torch.isfinite(xf).all(dim=-1) & torch.isfinite(twin).all(dim=-1)
    apart = float((xf - twin)[finite].abs().max().item()) if finite.any() and steps <= 100 else None
    out = {"step_nbr": steps, "samples_per_row": Q, "lanes": B * K, "call_ms": t_call, "composed_ms": t_comp, "composed_over_call": t_comp / t_call,
           "aim_composed_over_call_ge_1.0": "met" if t_comp / t_call >= 1.0 else "NOT met",
           "residual_ms": t_res, "call_over_residual": t_call / t_res, "open_loop_ms": t_open, "closed_over_open": t_call / t_open,
           "trajectories_per_s": B * K / (t_call * 1e-3),
           "call_ms_all": raw[0], "composed_ms_all": raw[1], "residual_ms_all": raw[2], "open_loop_ms_all": raw[3],
           "spread_ms": [max(r) - min(r) for r in raw],
           "corrections_per_case_median": float(nupd.float().median().item()), "skipped_per_case_median": float(nskip.float().median().item()),
           "miss_inf_median": float(miss.abs().amax(dim=-1).nanmedian().item()), "call_and_composed_xf_apart": apart}
    ctx.close()
    block.close()
    return out


result = {"B": B, "K": K, "M": 1, "d": D, "stride": args.stride, "every": 1, "sigma": args.sigma, "device": torch.cuda.get_device_name(0), "reps": 5}
for steps in args.steps:
    for variant in args.variants:
        for free_tf in (False, True):
            result["N%d_%s_%s" % (steps, variant, "free_tf" if free_tf else "fixed_tf")] = one(steps, variant, free_tf)
text = json.dumps(result, indent=1)
with open(args.out, "w") as f:
    f.write(text + "\n")
print(text)
