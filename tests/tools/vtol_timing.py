#!/usr/bin/env python3
"""vtolUAV workload of tests/testVtolUAV.cpp at its largest layout (M = 32 segments, n = 416 unknowns, 100 RK4 steps per segment,
nine boxes in the device-resident map): kernel time of one residual and one FD Jacobian from HIP events (device-resident
inputs and outputs, warm), the wall of the whole flow through the C++ mirror in both flavours, and of the 256-chain parameter
sweep of tests/test_gpu_vtol.py.  Run on the GPU box; prints one JSON object (kept in profiles/vtol_timing.json).  Beside it,
labelled as such, the reference's own wall for the same flow as recorded in the fixture on the machine that generated it."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from socp_amd import capi  # noqa: E402
import test_gpu_vtol as T  # noqa: E402

F = T.F
out = {}
ctx = capi.Context(capi.MODEL_VTOLUAV)
ctx.set_map(T.V["table_shipped"])
z0, _, zstar = T.stage_problem(ctx, "path_32")
n = len(z0)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
dz = torch.tensor(z0, device="cuda")
dF = torch.empty(n, dtype=torch.float64, device="cuda")
dJ = torch.empty(n * n, dtype=torch.float64, device="cuda")


def timed(fn, reps=10):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


for flavour, variant in (("exact", capi.VARIANT_LANE_EXACT), ("fast", capi.VARIANT_LANE_FAST)):
    ctx.set_variant(variant)
    out["residual_n416_%s_ms" % flavour] = timed(lambda: ctx.residual_batch_dev(1, dz.data_ptr(), dF.data_ptr()))
    for dedup in (False, True):
        out["fd_jacobian_n416_%s_%s_ms" % (flavour, "dedup" if dedup else "full")] = timed(
            lambda: ctx.fd_jacobian_dev(dz.data_ptr(), dF.data_ptr(), 1e-15, dJ.data_ptr(), dedup=dedup))
ctx.set_stream(0, use_own=True)
ctx.set_variant(capi.VARIANT_AUTO)

for variant in ("exact", "fast"):
    t = time.perf_counter()
    stages = T.run_flow([1e-10, 0, 60, 1], variant)
    out["flow_xtol1e-10_%s_wall_s" % variant] = time.perf_counter() - t
    out["flow_xtol1e-10_%s_nfev" % variant] = [s["nfev"] for s in stages]
out["reference_nfev"] = [int(v) for v in F["nfev"]]
out["reference_flow_wall_s_OTHER_MACHINE"] = {"wall_s": float(F["ref_wall_s"]), "cpu_s": float(F["ref_cpu_s"]), "machine": str(F["ref_machine"])}

# the 256-chain sweep: invSigmaXwp, then muObs, device solver
z8_0, _, z8 = T.stage_problem(ctx, "path_8", prefix="wp8_")
base = F["wp8_path_8_params"].copy()
sigma, mu = T.sweep_goals()
for name, solver in (("host", capi.SOLVER_HOST), ("device", capi.SOLVER_DEVICE)):
    t = time.perf_counter()
    P1 = np.tile(base, (T.K_CHAINS, 1))
    a = ctx.chains_solve(np.tile(z8, (T.K_CHAINS, 1)), kind=capi.CHAIN_PARAM, param_index=T.I_INVSIGMA, step=1.0, goal=1.0 / sigma, params=P1,
                         xtol=1e-10, solver=solver)
    P2 = P1.copy()
    P2[:, T.I_INVSIGMA] = 1.0 / sigma
    b = ctx.chains_solve(a["z"], kind=capi.CHAIN_PARAM, param_index=T.I_MU, step=1.0, goal=mu, params=P2, xtol=1e-10, solver=solver)
    out["sweep_256_chains_n104_solver_%s" % name] = {"wall_s": time.perf_counter() - t, "converged": int((b["info"] == 1).sum()),
                                                      "newton_solves": int(a["solves"].sum() + b["solves"].sum()),
                                                      "residual_evaluations": int(a["nfev_total"].sum() + b["nfev_total"].sum())}
print(json.dumps(out, indent=1))
