#!/usr/bin/env python3
"""Batched Newton polish (socp_newton_batch) timed three ways; writes one JSON object to profiles/newton_timing.json (--out PATH
for another place) and prints it.

    python tests/tools/newton_timing.py

(a) the _dev call against the same rounds composed from public pieces: socp_exact_jacobian_batch_dev, torch.linalg.solve, tensor
    operations for the trial points and the selection, socp_residual_batch_dev on rows x trials, and a host decision (the live count
    read back) per round.  Bar: composed / call >= 1.0, reported as met or NOT met per shape.
(b) what the compaction buys: the same batch with 90 % of its rows already within ftol, the host form (live slots only) against the
    _dev form (all B slots).  No bar; the expected floor -- the start plus the live share of the rounds' work -- is recorded beside it.
(c) one round against one socp_exact_jacobian_batch_dev call on the same rows.  No bar.

Workload: Goddard single shooting (n = 14), 13 107 rows, 100-step and 10^4-step trajectories, both flavours; every row is the
polished root moved by 1e-7 (relative, its own draw).  HIP events, warm-up first, the sides alternated in one process, median of 5,
all five kept."""
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
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--trials", type=int, default=4)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "newton_timing.json"))
args = ap.parse_args()
FTOL_NEVER, FTOL_B = 1e-300, 1e-9


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


def composed(ctx, B, n, dZ, rounds, trials, ftol):
    """The rounds of include/socp_hip.h ("Polishing a table of roots") from public pieces; every round runs on all B rows."""
    dev, f64 = "cuda", torch.float64
    y = dZ.view(B, n).clone()
    F0 = torch.empty(B, n, dtype=f64, device=dev)
    J = torch.empty(B, n * n, dtype=f64, device=dev)
    T = torch.empty(B, trials, n, dtype=f64, device=dev)
    FT = torch.empty(B, trials, n, dtype=f64, device=dev)
    ctx.residual_batch_dev(B, y.data_ptr(), F0.data_ptr())
    rn = F0.abs().max(dim=1).values
    status = torch.where(~torch.isfinite(rn), 5, torch.where(rn <= ftol, 1, 0)).to(torch.int32)
    sk = torch.tensor([2.0 ** -k for k in range(trials)], dtype=f64, device=dev)
    ck = 1.0 - sk / 4
    rows = torch.arange(B, device=dev)
    for _ in range(rounds):
        if int((status == 0).sum().item()) == 0:                   # the host decision
            break
        ctx.exact_jacobian_batch_dev(B, y.data_ptr(), J.data_ptr(), None)
        delta = torch.linalg.solve(J.view(B, n, n).transpose(1, 2), -F0)
        T.copy_(y[:, None, :] + sk[None, :, None] * delta[:, None, :])
        ctx.residual_batch_dev(B * trials, T.data_ptr(), FT.data_ptr())
        rk = FT.abs().max(dim=2).values
        ok = rk < ck[None, :] * rn[:, None]
        first = torch.where(ok.any(dim=1), ok.to(torch.int8).argmax(dim=1), 0)
        take = (status == 0) & ok.any(dim=1)
        status = torch.where((status == 0) & ~ok.any(dim=1), 3, status)
        y = torch.where(take[:, None], T[rows, first], y)
        F0 = torch.where(take[:, None], FT[rows, first], F0)
        rn = torch.where(take, rk[rows, first], rn)
        status = torch.where(take & (rn <= ftol), 1, status)
    return status, rn


def shape(B, steps):
    ctx = capi.Context(capi.MODEL_GODDARD)
    ctx.set_params(sweep.GODDARD_PARAMS)
    ctx.set_step_number(steps)
    sweep.goddard_single_shooting_problem(ctx)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    n = ctx.n
    r0 = ctx.newton_batch(np.array(sweep.goddard_starts(1, 0.0)), jac=2, ftol=FTOL_NEVER, rounds=30, trials=8)
    root = r0["z"][0]
    rng = np.random.default_rng(steps)
    Z = root[None, :] * (1.0 + 1e-7 * rng.uniform(-1.0, 1.0, size=(B, n)))
    Zb = Z.copy()
    Zb[rng.permutation(B)[: (9 * B) // 10]] = root                 # (b): nine rows in ten are the root itself
    dZ, dZb = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (Z, Zb))
    R, T = args.rounds, args.trials
    never = capi.newton_options(jac=2, ftol=FTOL_NEVER, rounds=R, trials=T)
    one = capi.newton_options(jac=2, ftol=FTOL_NEVER, rounds=1, trials=T)
    ninety = capi.newton_options(jac=2, ftol=FTOL_B, rounds=R, trials=T)
    wb = ctx.newton_work_bytes(B, never)
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    f = lambda *s: torch.empty(*s, dtype=torch.float64, device="cuda")  # noqa: E731
    i = lambda *s: torch.empty(*s, dtype=torch.int32, device="cuda")  # noqa: E731
    outs = [f(B * n), f(B * n), f(B), f(B), i(B), i(B), i(B), f(B * (R + 1))]
    dJ = f(B * n * n)
    host = {}
    out = {"n": n, "B": B, "step_nbr": steps, "rounds": R, "trials": T, "work_bytes": wb, "root_rnorm": float(r0["rnorm"][0])}
    for variant in ("exact", "fast"):
        ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)

        def call(o=never, z=dZ):
            ctx.newton_batch_dev(B, z.data_ptr(), o, work.data_ptr(), wb, *(a.data_ptr() for a in outs))
        kept = {}

        def compose():
            kept["status"], kept["rn"] = composed(ctx, B, n, dZ, R, T, FTOL_NEVER)

        def host_form():
            host["r"] = ctx.newton_batch(Zb, ninety, residual=False, history=False)
        (call_ms, comp_ms, round_ms, jac_ms, res_ms, dev90_ms, host90_ms), raw = median_ms(
            [call, compose, lambda: call(one), lambda: ctx.exact_jacobian_batch_dev(B, dZ.data_ptr(), dJ.data_ptr(), None),
             lambda: ctx.residual_batch_dev(B, dZ.data_ptr(), outs[1].data_ptr()), lambda: call(ninety, dZb), host_form])
        call()
        torch.cuda.synchronize()
        rn_call = outs[2].cpu().numpy()
        ratio = comp_ms / call_ms
        live_share = float(np.mean(host["r"]["iters"] > 0))
        out[variant] = {"call_ms": call_ms, "composed_ms": comp_ms, "composed_over_call": ratio, "bar_1.0": "met" if ratio >= 1.0 else "NOT met",
                        "rnorm_median_after_rounds": float(np.median(rn_call)), "composed_rnorm_median_after_rounds": float(kept["rn"].median().item()),
                        "status_histogram": np.bincount(outs[6].cpu().numpy(), minlength=6).tolist(),
                        "b_dev_all_slots_ms": dev90_ms, "b_host_live_slots_ms": host90_ms, "b_dev_over_host": dev90_ms / host90_ms,
                        "b_rows_with_a_step_share": live_share, "b_start_residual_ms": res_ms,
                        "b_expected_floor_ms": res_ms + 0.1 * (dev90_ms - res_ms),
                        "b_status_histogram": np.bincount(host["r"]["status"], minlength=6).tolist(),
                        "c_one_round_ms": round_ms, "c_exact_jacobian_ms": jac_ms, "c_round_over_jacobian": round_ms / jac_ms,
                        "call_ms_all": raw[0], "composed_ms_all": raw[1], "one_round_ms_all": raw[2], "exact_jacobian_ms_all": raw[3],
                        "b_dev_ms_all": raw[5], "b_host_ms_all": raw[6]}
    ctx.close()
    return out


result = {"device": torch.cuda.get_device_name(0), "reps": 5}
for steps in args.steps:
    result["goddard_n14_N%d" % steps] = shape(args.batch, steps)
    with open(args.out, "w") as fh:                                # kept after every shape: a later one may run long
        fh.write(json.dumps(result, indent=1) + "\n")
print(json.dumps(result, indent=1))
