#!/usr/bin/env python3
"""Row grouping (socp_group_batch_dev) on a sweep-sized table, and its first round against the same round written as PyTorch tensor
operations on the same device and the same table; writes one JSON object to profiles/group_timing.json (--out PATH for another
place) and prints it.

    python tests/tools/group_timing.py

B = 4 194 304 rows, n = 14 of ld = 16 columns (the trailing two hold NaN), synthetic tables with 1, 8 and 64 well-separated roots in
random order, relative noise 1e-9, plus 1 % rows with one entry that is not finite.  HIP events on the context's stream, warm-up
first, the sides alternated in one process, median of 7.  Per table:
  call_ms          the whole call, max_groups = 1024 (G rounds, the read-backs of the "next leader" word between their chunks included)
  one_group_ms     the whole call with max_groups = 1: the fill, the scan for the first leader, the FIRST round -- every row is
                   unassigned, it reads B n 8 bytes -- and the final count
  passes_ms        the same call with every row masked: the fill, the labels written, one round that returns at once, the count
  first_round_ms   one_group_ms - passes_ms: the first round alone, a difference of two medians
  torch_ms         ((V[:, :n] - l).abs() <= atol + rtol * l.abs()).all(1) with l = the first leader's row
The bar is ratio = torch_ms / one_group_ms >= 1.0: the call that CONTAINS the first round is held against the expression, so the
bar is not helped by the subtraction."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from socp_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=4194304)
ap.add_argument("--n", type=int, default=14)
ap.add_argument("--ld", type=int, default=16)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_timing.json"))
args = ap.parse_args()
B, n, ld, ATOL, RTOL = args.rows, args.n, args.ld, 0.0, 1e-6


def median_ms(fns, reps):
    """Median of `reps` event-timed calls of every function, alternated inside each repetition, after one untimed call of each."""
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


def table(G, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    i = torch.arange(n, device="cuda", dtype=torch.float64)
    roots = (1.0 + torch.arange(G, device="cuda", dtype=torch.float64))[:, None] * (1.0 + 0.01 * i)[None, :] * torch.where(i % 2 == 0, 1.0, -1.0)[None, :]
    pick = torch.randint(0, G, (B,), device="cuda", generator=gen)
    V = torch.full((B, ld), float("nan"), dtype=torch.float64, device="cuda")
    V[:, :n] = roots[pick] * (1.0 + 1e-9 * (2.0 * torch.rand((B, n), device="cuda", dtype=torch.float64, generator=gen) - 1.0))
    bad = torch.randint(1, B, (B // 100,), device="cuda", generator=gen)                 # (row 0 stays finite: it leads)
    V[bad, torch.randint(0, n, (B // 100,), device="cuda", generator=gen)] = float("inf")
    return V


ctx = capi.Context(capi.MODEL_GODDARD)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
CAP = 1024
label = torch.empty(B, dtype=torch.int32, device="cuda")
leader, count = torch.empty(CAP, dtype=torch.int32, device="cuda"), torch.empty(CAP, dtype=torch.int32, device="cuda")
radius, summary = torch.empty(CAP, dtype=torch.float64, device="cuda"), torch.empty(4, dtype=torch.int32, device="cuda")
nobody = torch.zeros(B, dtype=torch.int32, device="cuda")


def group(V, mask, max_groups):
    ctx.group_batch_dev(B, n, ld, V.data_ptr(), mask.data_ptr() if mask is not None else None, ATOL, RTOL, max_groups, label.data_ptr(),
                        leader.data_ptr(), count.data_ptr(), radius.data_ptr(), summary.data_ptr())


result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "B": B, "n": n, "ld": ld, "atol": ATOL, "rtol": RTOL,
          "first_round_bytes": B * n * 8, "bar": "torch_ms / one_group_ms >= 1.0", "tables": {}}
for G in (1, 8, 64):
    V = table(G, 100 + G)
    lead = V[0, :n].clone()
    keep = {}

    def expression():
        keep["near"] = ((V[:, :n] - lead).abs() <= ATOL + RTOL * lead.abs()).all(1)
    (call_ms, one_ms, passes_ms, torch_ms), raw = median_ms(
        [lambda: group(V, None, CAP), lambda: group(V, None, 1), lambda: group(V, nobody, 1), expression], args.reps)
    # what was timed is what was meant: the groups of the whole call, and the first round against the expression
    group(V, None, CAP)
    torch.cuda.synchronize()
    s = summary.cpu().numpy().tolist()
    counts = count[:s[0]].cpu().numpy()
    group(V, None, 1)
    torch.cuda.synchronize()
    expression()
    same = bool(torch.equal(label == 0, keep["near"]))
    first = one_ms - passes_ms
    result["tables"]["roots_%d" % G] = {
        "groups": s[0], "overflow": s[1], "not_finite": s[2], "count_min": int(counts.min()), "count_max": int(counts.max()),
        "first_round_equals_expression": same,
        "call_ms": call_ms, "one_group_ms": one_ms, "passes_ms": passes_ms, "first_round_ms": first, "torch_ms": torch_ms,
        "first_round_bytes_per_s": B * n * 8 / (first * 1e-3), "one_group_bytes_per_s": B * n * 8 / (one_ms * 1e-3),
        "ratio": torch_ms / one_ms, "ratio_first_round_alone": torch_ms / first, "bar_met": bool(torch_ms / one_ms >= 1.0),
        "call_ms_all": raw[0], "one_group_ms_all": raw[1], "passes_ms_all": raw[2], "torch_ms_all": raw[3]}
    del V
ctx.close()
text = json.dumps(result, indent=1)
with open(args.out, "w") as f:
    f.write(text + "\n")
print(text)
