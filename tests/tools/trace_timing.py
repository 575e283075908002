#!/usr/bin/env python3
"""Batched trace (socp_trace_batch_dev) timings on the GPU box; prints one JSON object (kept in profiles/trace_timing.json).

    python tests/tools/trace_timing.py                  every timing below
    python tests/tools/trace_timing.py --case stride1   ONE untimed trace call, for a counter run of its own:
        rocprofv3 --pmc WRITE_SIZE --output-format csv -d DIR -- python tests/tools/trace_timing.py --case stride1

Workload of the bar: Goddard single shooting (n = 14), 10^4 RK4 steps, B = 196 605 (the bench headline's trajectory count),
both flavours; stride >= step_nbr keeps two rows per segment, and the trace launches must take at most 1.10 x
socp_residual_batch_dev of the same B on the same build (same lane mapping, same integration).  HIP events, device-resident
buffers, warm-up first, the two sides alternated in one process, median of 5.
Recorded without a bar: stride 100 at that size and stride 1 at step_nbr = 1000, B = 4096, with the bytes the rows need
(kept rows x W x 8 + the counts) to set the counter run's WRITE_SIZE against; and 4096 single-shooting trajectories at stride
100 in one batch against the existing one-at-a-time path (integrate_dense_aux, then ONE eval_batch per quantity over the kept
rows -- already kinder than one launch per row), timed on 8 of them and scaled."""
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
ap.add_argument("--case", choices=["all", "stride1", "stride100", "two_rows"], default="all")
ap.add_argument("--variant", choices=["exact", "fast"], default="fast", help="flavour of a --case run")
ap.add_argument("--batch", type=int, default=196605)
args = ap.parse_args()

ctx = capi.Context(capi.MODEL_GODDARD)
ctx.set_params(sweep.GODDARD_PARAMS)
sweep.goddard_single_shooting_problem(ctx)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
W = ctx.trace_width()


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


def buffers(B, cap):
    Z = sweep.goddard_starts(B, 1e-3)
    dZ = torch.from_numpy(Z).cuda()
    dR = torch.empty(B * cap * W, dtype=torch.float64, device="cuda")
    dC = torch.empty(B, dtype=torch.int32, device="cuda")
    return Z, dZ, dR, dC


def trace_case(B, step_nbr, stride, variant):
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    ctx.set_step_number(step_nbr)
    cap = step_nbr // stride + 3
    Z, dZ, dR, dC = buffers(B, cap)
    return cap, dZ, dR, dC, (lambda: ctx.trace_batch_dev(B, dZ.data_ptr(), stride, cap, dR.data_ptr(), dC.data_ptr()))


CASES = {"stride1": (4096, 1000, 1), "stride100": (args.batch, 10000, 100), "two_rows": (args.batch, 10000, 10000)}
if args.case != "all":
    B, step_nbr, stride = CASES[args.case]
    cap, dZ, dR, dC, fn = trace_case(B, step_nbr, stride, args.variant)
    fn()
    torch.cuda.synchronize()
    kept = int(dC.sum().item())
    print(json.dumps({"case": args.case, "variant": args.variant, "B": B, "step_nbr": step_nbr, "stride": stride, "kept_rows": kept,
                      "algorithmic_bytes": kept * W * 8 + B * 4}))
    sys.exit(0)

out = {"B": args.batch, "row_width": W, "device": torch.cuda.get_device_name(0)}
for variant in ("exact", "fast"):
    B, step_nbr, stride = CASES["two_rows"]
    cap, dZ, dR, dC, trace = trace_case(B, step_nbr, stride, variant)
    dF = torch.empty(B * 14, dtype=torch.float64, device="cuda")
    (res_ms, trace_ms), raw = median_ms([lambda: ctx.residual_batch_dev(B, dZ.data_ptr(), dF.data_ptr()), trace])
    assert int(dC.min().item()) == int(dC.max().item()) == 2
    out["two_rows_%s" % variant] = {"step_nbr": step_nbr, "stride": stride, "residual_ms": res_ms, "trace_ms": trace_ms, "ratio": trace_ms / res_ms,
                                    "bar": 1.10, "met": bool(trace_ms <= 1.10 * res_ms), "residual_ms_all": raw[0], "trace_ms_all": raw[1]}
    del dR, dF
    for name in ("stride100", "stride1"):
        B, step_nbr, stride = CASES[name]
        cap, dZ, dR, dC, trace = trace_case(B, step_nbr, stride, variant)
        (ms,), raw = median_ms([trace])
        kept = int(dC.sum().item())
        out["%s_%s" % (name, variant)] = {"B": B, "step_nbr": step_nbr, "stride": stride, "cap": cap, "trace_ms": ms, "trace_ms_all": raw[0], "kept_rows": kept,
                                          "algorithmic_bytes": kept * W * 8 + B * 4, "row_bytes_per_s": kept * W * 8 / (ms * 1e-3)}
        del dR

# 4096 trajectories at stride 100: one batch against the one-at-a-time path on 8 of them
ctx.set_variant(capi.VARIANT_LANE_FAST)
ctx.set_step_number(10000)
ctx.set_stream(0, use_own=True)
Z = sweep.goddard_starts(4096, 1e-3)
ctx.trace_batch(Z[:8], stride=100)
t0 = time.perf_counter()
rows, count = ctx.trace_batch(Z, stride=100)
batch_s = time.perf_counter() - t0


def one_at_a_time(z):
    tl = ctx.timeline(z)
    t, X, aux = ctx.integrate_dense_aux(tl[0], tl[1], z[:14])
    kept = capi.trace_kept_rows(len(t), 100)
    u = ctx.eval_batch(capi.EVAL_CONTROL, t[kept], X[kept], sw=aux[kept])
    H = ctx.eval_batch(capi.EVAL_HAMILTONIAN, t[kept], X[kept], sw=aux[kept])
    return np.concatenate([t[kept, None], X[kept], u, H, aux[kept]], axis=1)


one_at_a_time(Z[0])
t0 = time.perf_counter()
singles = [one_at_a_time(z) for z in Z[:8]]
single_s = (time.perf_counter() - t0) / 8
same = all(np.array_equal(rows[b, 0, :count[b, 0]].view(np.uint64), singles[b].view(np.uint64)) for b in range(8))
out["batch_4096_stride100_fast"] = {"host_form_wall_s": batch_s, "one_at_a_time_wall_s_per_trajectory": single_s, "one_at_a_time_timed_on": 8,
                                    "one_at_a_time_wall_s_scaled_to_4096": single_s * 4096, "speed_up": single_s * 4096 / batch_s,
                                    "rows_of_the_8_equal_bitwise": bool(same), "inputs": "sweep.goddard_starts(4096, 1e-3): starts around the converged solution"}
print(json.dumps(out, indent=1))
