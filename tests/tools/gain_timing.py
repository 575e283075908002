#!/usr/bin/env python3
"""Batched neighbouring-extremal gains (socp_gain_batch_dev) on the GPU box beside the same job composed from the library's earlier
entry points: socp_regrid_batch_dev onto one segment per block, socp_fields_batch_dev with all columns for the transition matrix of
each, a torch product chain W <- W Phi, and torch.linalg.solve_ex for A_p K = -A_x (solve_ex: A_p is singular near the end of the
flight, where the thrust is off, and torch.linalg.solve would raise).  The aim is composed / call >= 1.0; the JSON says met or NOT met.
Writes one JSON object to profiles/gain_timing.json (--out PATH for another place) and prints it.

    python tests/tools/gain_timing.py

Workload: Goddard single shooting (n = 14, M = 1, d = 7), B = 13 107, stride 100, at 100 and 10^4 RK4 steps, both flavours, all sides
on the same device-resident Z.  HIP events, warm-up first, the sides alternated in one process, median of 5 with the spread.  The
share of the call that each of its three launches takes comes from the kernel records of torch.profiler over one more call."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gain_timing.json"))
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


def launch_shares(fn):
    """Device time of the call's three launches from the profiler's kernel records: dict(blocks, sweep, elimination) in ms, or None."""
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ms = {"blocks": 0.0, "sweep": 0.0, "elimination": 0.0}
        for e in prof.events():
            for key, tag in (("blocks", "gain_blocks_kernel"), ("sweep", "gain_sweep_kernel"), ("elimination", "linsolve_slots_kernel")):
                if tag in e.name:
                    ms[key] += getattr(e, "device_time", getattr(e, "cuda_time", 0.0)) / 1000.0
        return ms if sum(ms.values()) > 0 else None
    except Exception as err:                                          # no tracer on this box: the shares stay unmeasured
        return {"error": str(err)}


def one(steps, variant):
    Q = max(1, -(-steps // args.stride))
    ctx = capi.Context(capi.MODEL_GODDARD)
    ctx.set_params(sweep.GODDARD_PARAMS)
    ctx.set_step_number(steps)
    sweep.goddard_single_shooting_problem(ctx)
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    # the composed side's second context: one segment per block, `stride` steps each, every interior node CONTINUOUS
    seg = capi.Context(capi.MODEL_GODDARD)
    seg.set_params(sweep.GODDARD_PARAMS)
    seg.set_step_number(min(args.stride, steps))
    mode_x = np.zeros((Q + 1, D), dtype=np.int32)
    mode_x[1:Q] = capi.CONTINUOUS
    mode_x[Q, 3:7] = capi.FREE
    nodes = np.zeros((Q + 1, S))
    nodes[0, :7] = sweep.X0_STATE
    nodes[Q, 0] = 1.01
    times = np.array([sweep.TF * min(q * args.stride, steps) / steps for q in range(Q + 1)])
    assert seg.problem_set([capi.FIXED] * (Q + 1), mode_x, times, nodes) == S * Q
    seg.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    seg.set_stream(torch.cuda.current_stream().cuda_stream)

    f64 = dict(dtype=torch.float64, device=dev)
    dZ = torch.from_numpy(sweep.goddard_starts(B, 1e-3)).cuda()
    tq, kp = torch.empty((B, 1, Q), **f64), torch.empty((B, 1, Q, D, D), **f64)
    info = torch.zeros((B, 1, Q), dtype=torch.int32, device=dev)
    cnt = torch.zeros((B, 1), dtype=torch.int32, device=dev)
    T2 = torch.from_numpy(np.tile(times, (B, 1))).cuda()
    Z2 = torch.empty((B, S * Q), **f64)
    tq2, det2 = torch.empty((B, Q, 1), **f64), torch.empty((B, Q, 1), **f64)
    cnt2 = torch.zeros((B, Q), dtype=torch.int32, device=dev)
    nch2 = torch.zeros((B, Q), dtype=torch.int32, device=dev)
    tcj2 = torch.empty((B, Q), **f64)
    phi = torch.empty((B, Q, S, S), **f64)
    E = torch.zeros((D, S), **f64)
    for j in range(D):
        E[j, D + j if j >= 3 else j] = 1.0
    kept = {}

    def call():
        ctx.gain_batch_dev(B, dZ.data_ptr(), args.stride, Q, tq.data_ptr(), kp.data_ptr(), info.data_ptr(), cnt.data_ptr())

    def composed():
        ctx.regrid_batch_dev(B, dZ.data_ptr(), [capi.FIXED] * (Q + 1), T2.data_ptr(), Z2.data_ptr())
        seg.fields_batch_dev(B, Z2.data_ptr(), capi.FIELDS_ALL, args.stride, 0, 1, tq2.data_ptr(), det2.data_ptr(), cnt2.data_ptr(),
                             nch2.data_ptr(), tcj2.data_ptr(), phi.data_ptr())
        W = E.expand(B, D, S)
        Wq = torch.empty((B, Q, D, S), **f64)
        for q in range(Q - 1, -1, -1):
            W = torch.bmm(W, phi[:, q])
            Wq[:, q] = W
        kept["k"] = torch.linalg.solve_ex(Wq[..., D:], -Wq[..., :D])[0]

    (t_call, t_comp), raw = median_ms([call, composed])
    torch.cuda.synchronize()
    ok = info[:, 0] == 0
    k_call = kp.transpose(-1, -2)[:, 0]                                # kp is column-major
    scale = k_call[ok].abs().max().item() if ok.any() else float("nan")
    diff = (kept["k"] - k_call)[ok].abs().max().item() if ok.any() else float("nan")
    shares = launch_shares(call)
    out = {"step_nbr": steps, "blocks_per_row": Q, "call_ms": t_call, "composed_ms": t_comp, "composed_over_call": t_comp / t_call,
           "aim_composed_over_call_ge_1": "met" if t_comp / t_call >= 1.0 else "NOT met",
           "call_ms_all": raw[0], "composed_ms_all": raw[1], "call_spread_ms": max(raw[0]) - min(raw[0]),
           "composed_spread_ms": max(raw[1]) - min(raw[1]), "launch_ms": shares,
           "solved_samples": int(ok.sum().item()), "samples": int(ok.numel()),
           "composed_minus_call_max_over_scale": diff / scale if scale == scale and scale > 0 else None,
           "workspace_bytes": B * Q * (S * S + D * D) * 8}
    if isinstance(shares, dict) and "blocks" in shares:
        total = sum(shares.values())
        out["launch_share_of_call"] = {k: v / total for k, v in shares.items()}
    ctx.close()
    seg.close()
    return out


result = {"B": B, "M": 1, "d": D, "stride": args.stride, "device": torch.cuda.get_device_name(0), "reps": 5}
for steps in args.steps:
    for variant in ("exact", "fast"):
        result["N%d_%s" % (steps, variant)] = one(steps, variant)
text = json.dumps(result, indent=1)
with open(args.out, "w") as f:
    f.write(text + "\n")
print(text)
