#!/usr/bin/env python3
"""vtolUAV's exact shooting Jacobian (socp_exact_jacobian_batch_dev) on the GPU box beside socp_fd_jacobian_multi_dev -- the forward
difference all 36 solves of the waypoint flow run on -- on the same rows, in both flavours.  No bar: nothing else in the tree gives
an exact matrix for this model.  Writes one JSON object to profiles/vtol_exact_timing.json (--out PATH for another place) and
prints it.

    python tests/tools/vtol_exact_timing.py

Workload: stage path_32 of tests/golden/vtol_flow.npz (n = 416: 32 waypoint segments with FREE interior times, the shipped obstacle
map, the stored parameters), 100 RK4 steps per segment, B = 256 rows: the stored solution moved by up to 1e-3 relative.  Both sides on
the same context and the same device-resident Z (the forward difference at (z, F(z)) with F from socp_residual_batch_dev of the
context's own flavour; epsfcn 1e-15).  HIP events, a warm-up first, the sides alternated in one process, median of 5 with the
spread.  The exact kernel is one reference-order object for both flavours: a flavour changes only the forward-difference side."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from socp_amd import capi  # noqa: E402
import vtol_exact_reference as vx  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--stage", default="path_32")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vtol_exact_timing.json"))
args = ap.parse_args()

GOLD = os.path.join(ROOT, "tests", "golden")
P, prob, z = vx.stage(np.load(os.path.join(GOLD, "vtol_flow.npz")), args.stage)
table = np.load(os.path.join(GOLD, "vtol_vectors.npz"))["table_shipped"]
ctx = capi.Context(capi.MODEL_VTOLUAV)
ctx.set_exact_hooks(True)
ctx.set_map(table)
ctx.set_params(P)
ctx.set_step_number(args.steps)
n = ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)


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
    return [float(np.median(t)) for t in times], times


B = args.batch
Z = np.tile(z, (B, 1)) * (1.0 + 1e-3 * np.random.default_rng(7).uniform(-1.0, 1.0, size=(B, n)))
Z[0] = z
dZ = torch.from_numpy(Z).cuda()
dJ = torch.empty((B, n * n), dtype=torch.float64, device="cuda")
dJfd = torch.empty((B, n * n), dtype=torch.float64, device="cuda")
dF = torch.empty((B, n), dtype=torch.float64, device="cuda")          # the exact call's F: the reference-order residual
dFfd = torch.empty((B, n), dtype=torch.float64, device="cuda")        # the forward difference's F: the context's own flavour


def exact():
    ctx.exact_jacobian_batch_dev(B, dZ.data_ptr(), dJ.data_ptr(), dF.data_ptr())


def fd():
    ctx.fd_jacobian_multi_dev(B, dZ.data_ptr(), dFfd.data_ptr(), 1e-15, dJfd.data_ptr())


out = {"stage": args.stage, "B": B, "M": int(prob.M), "d": 6, "n": int(n), "step_nbr": args.steps, "obstacles": int(len(table)),
       "device": torch.cuda.get_device_name(0), "reps": args.reps, "runs": []}
for variant in ("exact", "fast"):
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    ctx.residual_batch_dev(B, dZ.data_ptr(), dFfd.data_ptr())
    (e, f), raw = median_ms([exact, fd], args.reps)
    torch.cuda.synchronize()
    big = dJ.abs().amax(dim=1)
    dev_fd = (dJfd - dJ).abs().amax(dim=1) / big
    out["runs"].append({"variant": variant, "exact_jacobian_ms": e, "fd_jacobian_ms": f, "exact_over_fd": e / f,
                        "exact_jacobian_ms_all": raw[0], "fd_jacobian_ms_all": raw[1],
                        "exact_jacobian_ms_spread": [min(raw[0]), max(raw[0])], "fd_jacobian_ms_spread": [min(raw[1]), max(raw[1])],
                        "fd_dev_median": float(dev_fd.nanmedian().item()), "fd_dev_max": float(dev_fd[torch.isfinite(dev_fd)].max().item()),
                        "rows_finite": int(torch.isfinite(dJ).all(dim=1).sum().item())})
text = json.dumps(out, indent=1)
with open(args.out, "w") as f:
    f.write(text + "\n")
print(text)
