#!/usr/bin/env python3
"""Batched extrema (socp_extrema_batch_dev) timings on the GPU box; writes one JSON object (kept in profiles/extrema_timing.json).

    python tests/tools/extrema_timing.py [--out PATH]

Workload: Goddard single shooting (n = 14, M = 1), B = 13 107 starts around the converged solution, at 1000 and at 10^4 RK4 steps,
both flavours.  HIP events, device-resident buffers, warm-up first, the sides alternated in one process, median of 5 with the
smallest and the largest.
The bar: the call with what = 7 against the composition it replaces -- socp_trace_batch_dev with stride = 1 and cap = N + 1, then
torch.amin / amax / argmin / argmax over the rows of the t, X, u, H columns (the composition has no event channel: it does LESS
than the call, which also reduces the switching function) -- composed / call >= 1.0.  At N = 10^4 the composition's rows take
22 GB; when that allocation fails the fact is recorded and N = 1000 stands alone.
Without a bar: the call with what = 0 and what = 7 against a residual launch of the same trajectories -- what carrying the
running pairs, and evaluating u, H and g at every step, costs."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extrema_timing.json"))
ap.add_argument("--batch", type=int, default=13107)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()

ctx = capi.Context(capi.MODEL_GODDARD)
ctx.set_params(sweep.GODDARD_PARAMS)
sweep.goddard_single_shooting_problem(ctx)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
W, Cw, B = ctx.trace_width(), ctx.extrema_width(), args.batch
S, NU = 14, 3


def median_ms(fns, reps):
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
    return [dict(median_ms=float(np.median(t)), min_ms=float(min(t)), max_ms=float(max(t)), all_ms=t) for t in times]


def one_size(N, variant):
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    ctx.set_step_number(N)
    dZ = torch.from_numpy(sweep.goddard_starts(B, 1e-3)).cuda()
    lo, hi, ta, tb = (torch.empty(B * Cw, dtype=torch.float64, device="cuda") for _ in range(4))
    cnt, bad = (torch.empty(B, dtype=torch.int32, device="cuda") for _ in range(2))
    dF = torch.empty(B * 14, dtype=torch.float64, device="cuda")

    def call(what):
        return lambda: ctx.extrema_batch_dev(B, dZ.data_ptr(), what, lo.data_ptr(), hi.data_ptr(), ta.data_ptr(), tb.data_ptr(), cnt.data_ptr(),
                                             bad.data_ptr())
    fns = [lambda: ctx.residual_batch_dev(B, dZ.data_ptr(), dF.data_ptr()), call(0), call(7)]
    names = ["residual", "extrema_what0", "extrema_what7"]
    cap = N + 1
    rec = {"step_nbr": N, "trace_rows_bytes": B * cap * W * 8}
    try:
        dR = torch.empty((B, cap, W), dtype=torch.float64, device="cuda")
        dC = torch.empty(B, dtype=torch.int32, device="cuda")
        keep = {}

        def composed():
            ctx.trace_batch_dev(B, dZ.data_ptr(), 1, cap, dR.data_ptr(), dC.data_ptr())
            v = dR[:, :, 1:1 + S + NU + 1]
            keep["vmin"], keep["vmax"] = torch.amin(v, dim=1), torch.amax(v, dim=1)
            keep["tmin"] = torch.gather(dR[:, :, 0], 1, torch.argmin(v, dim=1))
            keep["tmax"] = torch.gather(dR[:, :, 0], 1, torch.argmax(v, dim=1))
        composed()                                   # the reductions' own temporaries are part of what must fit
        torch.cuda.synchronize()
        fns.append(composed)
        names.append("composed")
    except torch.OutOfMemoryError as exc:
        rec["composed"] = "the allocation of the rows failed: %s" % str(exc).splitlines()[0]
    for name, r in zip(names, median_ms(fns, args.reps)):
        rec[name] = r
    assert int(cnt.min().item()) == int(cnt.max().item()) == N + 1 and int(bad.sum().item()) == 0
    if "composed" in names:
        # the two sides agree where both are defined (exact flavour: bit for bit; throughput flavour: two contractions)
        assert int(dC.min().item()) == int(dC.max().item()) == N + 1
        a, b = lo.view(B, Cw)[:, :S + NU + 1], keep["vmin"]
        rec["max_abs_difference_of_vmin"] = float((a - b).abs().max().item())
        ratio = rec["composed"]["median_ms"] / rec["extrema_what7"]["median_ms"]
        rec["composed_over_call"] = ratio
        rec["bar"] = 1.0
        rec["met"] = bool(ratio >= 1.0)
    for what in ("what0", "what7"):
        rec["extrema_%s_over_residual" % what] = rec["extrema_" + what]["median_ms"] / rec["residual"]["median_ms"]
    return rec


out = {"B": B, "M": 1, "channels": Cw, "trace_row_width": W, "device": torch.cuda.get_device_name(0), "reps": args.reps}
for variant in ("exact", "fast"):
    for N in (1000, 10000):
        out["%s_N%d" % (variant, N)] = one_size(N, variant)
        torch.cuda.empty_cache()
        r = out["%s_N%d" % (variant, N)]
        print("%s N = %d: residual %.2f ms, extrema what 0 %.2f ms, what 7 %.2f ms, composed %s ms: composed / call %s -> %s" % (
            variant, N, r["residual"]["median_ms"], r["extrema_what0"]["median_ms"], r["extrema_what7"]["median_ms"],
            "%.2f" % r["composed"]["median_ms"] if isinstance(r.get("composed"), dict) else "n/a",
            "%.2f" % r["composed_over_call"] if "composed_over_call" in r else "n/a",
            ("met" if r["met"] else "NOT met") if "met" in r else "no bar at this size"), flush=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
ctx.close()
