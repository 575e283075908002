#!/usr/bin/env python3
"""A model written from its Hamiltonian alone timed beside the hand-written one, and the Hamiltonian-gradient call beside the
evaluation of the right-hand side; writes one JSON object to profiles/hamiltonian_model_timing.json (--out PATH for another place)
and prints it.

    python tests/tools/hamiltonian_model_timing.py

(1) One residual launch (socp_residual_batch_dev) of tests/plugin/dint_h_plugin.hip against the in-tree double integrator on the same
    rows: testDoubleIntegrator's problem (M = 1, free tf, n = 13), 13 107 rows, 100 and 1000 RK4 steps.
(2) socp_hamiltonian_gradient_batch against socp_eval_batch(SOCP_EVAL_RHS) at 10^6 points, both host forms (they stage the same
    bytes up and down), and the gradient's _dev form alone, for the double integrator and Goddard's smooth law.
No bar: nothing in the tree did either before.  What the operation count predicts stands beside the numbers: a right-hand side by
dual numbers costs (1 + S) x the operations of H -- the value part once and S derivative parts, none of which the compiler may drop
(a seed's 0.0 times a value keeps its sign and its NaN) -- against the hand-written right-hand side's own count.

HIP events, warm-up first, the sides alternated in one process, median of 5, all five kept."""
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

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=13107)
ap.add_argument("--steps", type=int, nargs="+", default=[100, 1000])
ap.add_argument("--points", type=int, default=1000000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hamiltonian_model_timing.json"))
args = ap.parse_args()
PLUGIN = os.path.join(ROOT, "socp_amd", "_build", "plugins", "libdint_h_plugin.so")
DINT_H_ID = 1009


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


def residual_shape(B, steps):
    import jacobi_cases as jc
    c = jc.dint()
    prob = c["prob"]
    Z = np.ascontiguousarray(jc.perturbed(c["Z"][0], B, 0.05, seed=steps))
    dZ = torch.from_numpy(Z).cuda()
    ctxs, outs = [], []
    for model_id in (capi.MODEL_DOUBLE_INTEGRATOR, DINT_H_ID):
        ctx = capi.Context(model_id, nparams=3)
        ctx.set_params(np.asarray(c["params"], dtype=np.float64))
        ctx.set_step_number(steps)
        assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == prob.n
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctxs.append(ctx)
        outs.append(torch.empty(B * prob.n, dtype=torch.float64, device="cuda"))
    (hand_ms, h_ms), raw = median_ms([lambda k=k: ctxs[k].residual_batch_dev(B, dZ.data_ptr(), outs[k].data_ptr()) for k in (0, 1)])
    gap = float((outs[0] - outs[1]).abs().max())
    for ctx in ctxs:
        ctx.close()
    return {"B": B, "n": prob.n, "M": prob.M, "step_nbr": steps, "hand_written_ms": hand_ms, "from_hamiltonian_ms": h_ms,
            "from_hamiltonian_over_hand_written": h_ms / hand_ms, "max_abs_residual_gap": gap, "hand_written_ms_all": raw[0],
            "from_hamiltonian_ms_all": raw[1]}


def gradient_shape(model_id, params, X):
    B, S = X.shape
    ctx = capi.Context(model_id)
    ctx.set_params(np.asarray(params, dtype=np.float64))
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    t = np.zeros(B)
    dt, dX, dG = torch.from_numpy(t).cuda(), torch.from_numpy(X).cuda(), torch.empty(B * S, dtype=torch.float64, device="cuda")
    (grad_ms, rhs_ms, dev_ms), raw = median_ms([lambda: ctx.hamiltonian_gradient_batch(t, X), lambda: ctx.eval_batch(capi.EVAL_RHS, t, X),
                                                lambda: ctx.hamiltonian_gradient_batch_dev(B, dt.data_ptr(), None, dX.data_ptr(), dG.data_ptr())])
    ctx.close()
    return {"B": B, "S": S, "gradient_host_ms": grad_ms, "eval_rhs_host_ms": rhs_ms, "gradient_dev_ms": dev_ms,
            "gradient_over_eval_rhs_host": grad_ms / rhs_ms, "predicted_operations": "(1 + S) = %d x the operations of H per point" % (1 + S),
            "gradient_host_ms_all": raw[0], "eval_rhs_host_ms_all": raw[1], "gradient_dev_ms_all": raw[2]}


capi.plugin_load(PLUGIN)
result = {"device": torch.cuda.get_device_name(0), "reps": 5,
          "prediction": "a right-hand side by dual numbers costs (1 + S) x the operations of H; S = 12 for the double integrator: 13 x"}
for steps in args.steps:
    result["residual_dint_N%d" % steps] = residual_shape(args.batch, steps)
    with open(args.out, "w") as fh:                                # kept after every shape: a later one may run long
        fh.write(json.dumps(result, indent=1) + "\n")
rng = np.random.default_rng(1)
Xd = rng.uniform(-1.0, 1.0, size=(args.points, 12)) * rng.choice([0.3, 3.0], size=(args.points, 1))
result["gradient_dint"] = gradient_shape(capi.MODEL_DOUBLE_INTEGRATOR, [1.0, 1.0, 0.01], np.ascontiguousarray(Xd))
X0 = np.array([0.999949994, 1e-4, 0.01, 0.01, 0.02, -0.015, 1.0, -8.121947733, 7.775439382e-3, 0.7775438809, -0.4779369965, 5.715013318e-4,
               5.715009222e-2, 9.958404873e-2])
Xg = X0[None, :] * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, size=(args.points, 14)))
result["gradient_goddard_smooth"] = gradient_shape(capi.MODEL_GODDARD, [3.5, 7.0, 310.0, 500.0, 1.0, 1.0, 1.0, -1.0], np.ascontiguousarray(Xg))
with open(args.out, "w") as fh:
    fh.write(json.dumps(result, indent=1) + "\n")
print(json.dumps(result, indent=1))
