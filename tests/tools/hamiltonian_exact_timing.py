#!/usr/bin/env python3
"""The Jacobian of the Hamiltonian vector field timed beside the composition it replaces, and the exact entries of a model written from
its Hamiltonian alone beside the hand-written model's; writes one JSON object to profiles/hamiltonian_exact_timing.json (--out PATH
for another place) and prints it.

    python tests/tools/hamiltonian_exact_timing.py

(a) socp_hamiltonian_jacobian_batch_dev at 10^6 points against the composition it replaces: S + 1 calls of
    socp_hamiltonian_gradient_batch_dev (the point and its S perturbed copies, formed by torch) and the torch difference that fills
    A.  The ratio composed / call is reported against a bar of 1.0, met or NOT met; the double integrator and Goddard's smooth law.
(b) socp_exact_jacobian_batch_dev of tests/plugin/dint_hx_plugin.hip against the in-tree double integrator on the same rows:
    testDoubleIntegrator's problem (M = 1, free tf, n = 13), 13 107 rows, 100 and 1000 RK4 steps.  No bar.  The operation count
    predicts (1 + S) Hamiltonian evaluations on nested numbers per right-hand side over dual numbers.
(c) One residual launch of dint_hx against dint_h (tests/plugin/dint_h_plugin.hip): the plain path of the exact adaptor is the plain
    adaptor's.

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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hamiltonian_exact_timing.json"))
args = ap.parse_args()
PLUGINS = os.path.join(ROOT, "socp_amd", "_build", "plugins")
DINT_H_ID, DINT_HX_ID = 1009, 1011


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


def spread(t):
    return (max(t) - min(t)) / float(np.median(t))


def point_shape(model_id, params, X, h=1e-6):
    B, S = X.shape
    ctx = capi.Context(model_id)
    ctx.set_params(np.asarray(params, dtype=np.float64))
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    dt, dX = torch.zeros(B, dtype=torch.float64, device="cuda"), torch.from_numpy(X).cuda()
    dA = torch.empty((B, S, S), dtype=torch.float64, device="cuda")
    dA2 = torch.empty((B, S, S), dtype=torch.float64, device="cuda")
    dG0, dG1 = torch.empty((B, S), dtype=torch.float64, device="cuda"), torch.empty((B, S), dtype=torch.float64, device="cuda")

    def call():
        ctx.hamiltonian_jacobian_batch_dev(B, dt.data_ptr(), None, dX.data_ptr(), dA.data_ptr(), None)

    def composed():
        ctx.hamiltonian_gradient_batch_dev(B, dt.data_ptr(), None, dX.data_ptr(), dG0.data_ptr())
        for j in range(S):
            Xj = dX.clone()
            Xj[:, j] += h
            ctx.hamiltonian_gradient_batch_dev(B, dt.data_ptr(), None, Xj.data_ptr(), dG1.data_ptr())
            dA2[:, j, :] = (dG1 - dG0) / h                        # column j of the column-major matrix

    (call_ms, comp_ms), raw = median_ms([call, composed])
    gap = float((dA - dA2).abs().max() / dA.abs().max())
    ctx.close()
    ratio = comp_ms / call_ms
    return {"B": B, "S": S, "call_ms": call_ms, "composed_ms": comp_ms, "composed_over_call": ratio, "bar": 1.0,
            "bar_met": "met" if ratio >= 1.0 else "NOT met", "forward_difference_step": h, "max_rel_gap_to_forward_differences": gap,
            "call_spread": spread(raw[0]), "composed_spread": spread(raw[1]), "call_ms_all": raw[0], "composed_ms_all": raw[1]}


def shooting_contexts(ids, steps):
    import jacobi_cases as jc
    c = jc.dint()
    prob = c["prob"]
    ctxs = []
    for model_id in ids:
        ctx = capi.Context(model_id, nparams=3)
        ctx.set_params(np.asarray(c["params"], dtype=np.float64))
        ctx.set_step_number(steps)
        assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == prob.n
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctxs.append(ctx)
    Z = np.ascontiguousarray(jc.perturbed(c["Z"][0], args.batch, 0.05, seed=steps))
    return prob, ctxs, torch.from_numpy(Z).cuda()


def exact_jacobian_shape(B, steps):
    prob, ctxs, dZ = shooting_contexts((capi.MODEL_DOUBLE_INTEGRATOR, DINT_HX_ID), steps)
    n = prob.n
    outs = [torch.empty(B * n * n, dtype=torch.float64, device="cuda") for _ in ctxs]
    (hand_ms, hx_ms), raw = median_ms([lambda k=k: ctxs[k].exact_jacobian_batch_dev(B, dZ.data_ptr(), outs[k].data_ptr(), None) for k in (0, 1)])
    gap = float((outs[0] - outs[1]).abs().max())
    for ctx in ctxs:
        ctx.close()
    return {"B": B, "n": n, "M": prob.M, "step_nbr": steps, "hand_written_ms": hand_ms, "from_hamiltonian_exact_ms": hx_ms,
            "from_hamiltonian_exact_over_hand_written": hx_ms / hand_ms, "max_abs_jacobian_gap": gap, "hand_written_spread": spread(raw[0]),
            "from_hamiltonian_exact_spread": spread(raw[1]), "hand_written_ms_all": raw[0], "from_hamiltonian_exact_ms_all": raw[1]}


def residual_shape(B, steps):
    prob, ctxs, dZ = shooting_contexts((DINT_H_ID, DINT_HX_ID), steps)
    outs = [torch.empty(B * prob.n, dtype=torch.float64, device="cuda") for _ in ctxs]
    (h_ms, hx_ms), raw = median_ms([lambda k=k: ctxs[k].residual_batch_dev(B, dZ.data_ptr(), outs[k].data_ptr()) for k in (0, 1)])
    same = bool(torch.equal(outs[0], outs[1]))
    for ctx in ctxs:
        ctx.close()
    return {"B": B, "n": prob.n, "step_nbr": steps, "dint_h_ms": h_ms, "dint_hx_ms": hx_ms, "dint_hx_over_dint_h": hx_ms / h_ms,
            "same_bits": same, "dint_h_spread": spread(raw[0]), "dint_hx_spread": spread(raw[1]), "dint_h_ms_all": raw[0], "dint_hx_ms_all": raw[1]}


def keep(result):
    with open(args.out, "w") as fh:                                # kept after every shape: a later one may run long
        fh.write(json.dumps(result, indent=1) + "\n")


for name in ("libdint_h_plugin.so", "libdint_hx_plugin.so"):
    capi.plugin_load(os.path.join(PLUGINS, name))
result = {"device": torch.cuda.get_device_name(0), "reps": 5,
          "prediction": "a right-hand side over dual numbers by nested numbers costs (1 + S) Hamiltonian evaluations on numbers of "
                        "2 (1 + W) doubles; S = 12 for the double integrator"}
rng = np.random.default_rng(1)
Xd = rng.uniform(-1.0, 1.0, size=(args.points, 12)) * rng.choice([0.3, 3.0], size=(args.points, 1))
result["point_call_dint"] = point_shape(capi.MODEL_DOUBLE_INTEGRATOR, [1.0, 1.0, 0.01], np.ascontiguousarray(Xd))
keep(result)
X0 = np.array([0.999949994, 1e-4, 0.01, 0.01, 0.02, -0.015, 1.0, -8.121947733, 7.775439382e-3, 0.7775438809, -0.4779369965, 5.715013318e-4,
               5.715009222e-2, 9.958404873e-2])
Xg = X0[None, :] * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, size=(args.points, 14)))
result["point_call_goddard_smooth"] = point_shape(capi.MODEL_GODDARD, [3.5, 7.0, 310.0, 500.0, 1.0, 1.0, 1.0, -1.0], np.ascontiguousarray(Xg))
keep(result)
for steps in args.steps:
    result["residual_dint_hx_N%d" % steps] = residual_shape(args.batch, steps)
    keep(result)
    result["exact_jacobian_dint_hx_N%d" % steps] = exact_jacobian_shape(args.batch, steps)
    keep(result)
print(json.dumps(result, indent=1))
