#!/usr/bin/env python3
"""Batched Move(tf) / re-grid (socp_move_batch_dev, socp_regrid_batch) timings on the GPU box; prints one JSON object (kept in
profiles/move_timing.json).

    python tests/tools/move_timing.py                every timing below
    python tests/tools/move_timing.py --case move    ONE untimed move call, for a counter run of its own:
        rocprofv3 --pmc WRITE_SIZE --output-format csv -d DIR -- python tests/tools/move_timing.py --case move

Workload of the bar: Goddard single shooting (M = 1, n = 14), 10^4 RK4 steps, B = 13 107 solutions, K = 15 query times each
(196 605 lanes, the bench headline's trajectory count), both flavours.  With M = 1 every query starts from node 0, so
socp_integrate_batch_dev over the identical (t0, tf, X0) triples is the same integration loop without the move's prologue, and the
move must take at most 1.10 x of it on the same build.  HIP events, device-resident buffers, warm-up first, the two sides alternated
in one process, median of 5.  The two outputs are compared too (bit for bit in the reference-order flavour).
Recorded without a bar: a re-grid of 4096 M = 6 solutions onto the stage-4 structure of the testGoddard flow (host form, wall
clock) against the same work done one solution at a time through move_batch(B = 1), timed on 16 of them and scaled."""
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
ap.add_argument("--case", choices=["all", "move"], default="all")
ap.add_argument("--variant", choices=["exact", "fast"], default="fast", help="flavour of a --case run")
ap.add_argument("--solutions", type=int, default=13107)
ap.add_argument("--queries", type=int, default=15)
ap.add_argument("--steps", type=int, default=10000)
args = ap.parse_args()

S = 14
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


B, K = args.solutions, args.queries
lanes = B * K
Z = sweep.goddard_starts(B, 1e-3)
TQ = np.tile(sweep.TF * (np.arange(K) + 1.0) / K, (B, 1))
dZ, dQ = torch.from_numpy(Z).cuda(), torch.from_numpy(TQ).cuda()
dXm = torch.empty(lanes * S, dtype=torch.float64, device="cuda")
# the identical triples for the trajectory batch: t0 = tl(0) = 0, tf = the query, X0 = node 0 of the row
dT0 = torch.zeros(lanes, dtype=torch.float64, device="cuda")
dX0 = dZ[:, :S].repeat_interleave(K, dim=0).contiguous()
dXi = torch.empty(lanes * S, dtype=torch.float64, device="cuda")


def move():
    ctx.move_batch_dev(B, dZ.data_ptr(), K, dQ.data_ptr(), dXm.data_ptr(), None)


def integrate():
    ctx.integrate_batch_dev(lanes, dT0.data_ptr(), dQ.data_ptr(), None, dX0.data_ptr(), dXi.data_ptr())


if args.case == "move":
    ctx.set_variant(capi.VARIANT_LANE_FAST if args.variant == "fast" else capi.VARIANT_LANE_EXACT)
    move()
    torch.cuda.synchronize()
    print(json.dumps({"case": "move", "variant": args.variant, "lanes": lanes, "step_nbr": args.steps,
                      "algorithmic_bytes_written": lanes * S * 8, "algorithmic_bytes_read": B * S * 8 + lanes * 8}))
    sys.exit(0)

out = {"solutions": B, "queries": K, "lanes": lanes, "step_nbr": args.steps, "device": torch.cuda.get_device_name(0)}
for variant in ("exact", "fast"):
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    (int_ms, move_ms), raw = median_ms([integrate, move])
    a, b = dXm.cpu().numpy(), dXi.cpu().numpy()
    out["move_%s" % variant] = {"integrate_ms": int_ms, "move_ms": move_ms, "ratio": move_ms / int_ms, "bar": 1.10, "met": bool(move_ms <= 1.10 * int_ms),
                                "integrate_ms_all": raw[0], "move_ms_all": raw[1], "outputs_equal_bitwise": bool(np.array_equal(a.view(np.uint64), b.view(np.uint64))),
                                "outputs_max_rel_deviation": float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))}

# re-grid of 4096 M = 6 solutions (the golden stage-3 solution of the testGoddard flow, costates perturbed) in one batch against
# one solution at a time
gold = json.load(open(os.path.join(ROOT, "tests", "golden", "goddard_flow.json")))["goddard_N10_M6"][2]["z"]
g = capi.Context(capi.MODEL_GODDARD)
g.set_params([3.5, 7.0, 310.0, 500.0, 1.0, 1.0, 0.2, -1.0])
g.set_step_number(10)
g.set_variant(capi.VARIANT_LANE_FAST)
sweep.goddard_multiple_shooting_problem(g, 6)
P = 4096
rng = np.random.default_rng(1)
Z6 = np.tile(np.array(gold), (P, 1))
Z6[:, 7:14] *= 1.0 + 1e-4 * rng.uniform(-1, 1, (P, 7))
tf = Z6[0, -1]
mode_t2 = [capi.FIXED, capi.CONTINUOUS, capi.FREE, capi.CONTINUOUS, capi.FREE, capi.CONTINUOUS, capi.FREE]
T2 = np.tile([0.0, 0.0227 / 2, 0.0227, (0.08 + 0.0227) / 2, 0.08, (0.08 + tf) / 2, tf], (P, 1))
g.regrid_batch(Z6[:8], mode_t2, T2[:8])
t0 = time.perf_counter()
r = g.regrid_batch(Z6, mode_t2, T2)
batch_s = time.perf_counter() - t0


def one_at_a_time(z, t2):
    X = g.move_batch(z[None, :], t2[None, :])[0]
    return np.concatenate([X[:6].ravel(), t2[[2, 4, 6]]]), X


one_at_a_time(Z6[0], T2[0])
t0 = time.perf_counter()
singles = [one_at_a_time(Z6[b], T2[b]) for b in range(16)]
single_s = (time.perf_counter() - t0) / 16
same = all(np.array_equal(r["z"][b].view(np.uint64), singles[b][0].view(np.uint64)) and
           np.array_equal(r["xnode"][b].view(np.uint64), singles[b][1].view(np.uint64)) for b in range(16))
out["regrid_4096_M6_fast"] = {"step_nbr": 10, "host_form_wall_s": batch_s, "one_at_a_time_wall_s_per_solution": single_s, "one_at_a_time_timed_on": 16,
                              "one_at_a_time_wall_s_scaled_to_4096": single_s * P, "speed_up": single_s * P / batch_s,
                              "results_of_the_16_equal_bitwise": bool(same)}
print(json.dumps(out, indent=1))
