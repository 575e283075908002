#!/usr/bin/env python3
"""Writes tests/golden/vtol_exact_pin.npz: what tests/test_gpu_vtol_exact.py holds the vtolUAV exact Jacobian to, computed by
tests/vtol_exact_reference.py alone (no GPU, no library).

    python tests/golden/make_vtol_exact_golden.py

Per stage (path_1, path_2 of vtol_flow.npz at their stored solutions, ca = alphaV = 0.05, N = 10 steps) and per map (the shipped
table, an EMPTY table): the 240-bit matrix rounded to doubles, the double-precision restatement's deviation from it as a share of
max|J| (dev_ref), the decision margins; per stage, with the shipped map: the Newton starts z* + factor max(1, |z*|) xi and the
restatement's Newton results.  Data only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import vtol_exact_reference as vx          # noqa: E402
from fast_reference import mpmath          # noqa: E402

NEWTON_FACTOR = 1e-5                        # test_vtol_exact_cpu.py: every start converges with the issue's factor


def main():
    mpmath.mp.prec = 240
    flow = np.load(os.path.join(HERE, "vtol_flow.npz"))
    shipped = np.load(os.path.join(HERE, "vtol_vectors.npz"))["table_shipped"]
    out = dict(table_shipped=shipped, table_empty=np.zeros((0, 7)), N=np.int32(vx.N_STEPS), newton_factor=np.float64(NEWTON_FACTOR),
               stages=np.array(vx.STAGES))
    for name in vx.STAGES:
        P, prob, z = vx.stage(flow, name, ca=vx.CA, alphaV=vx.ALPHAV)
        out[name + "_params"], out[name + "_z"] = P, z
        out[name + "_mode_t"] = np.asarray(prob.mode_t, dtype=np.int32)
        out[name + "_mode_x"] = np.asarray(prob.mode_x, dtype=np.int32)
        out[name + "_time"], out[name + "_xnode"] = np.asarray(prob.time, dtype=np.float64), np.asarray(prob.xnode, dtype=np.float64)
        for tag, table in (("shipped", shipped), ("empty", out["table_empty"])):
            margins = {}
            J, F = vx.exact_jacobian_row(P, table, prob, z, vx.N_STEPS, margins=margins)
            Jh, Fh = vx.exact_jacobian_row(P, table, prob, z, vx.N_STEPS, high=True)
            key = "%s_%s_" % (name, tag)
            out[key + "J240"], out[key + "F240"] = vx.to_double(Jh), vx.to_double(Fh)
            out[key + "dev_ref"] = np.float64(vx.dev_of(J, Jh))
            out[key + "margins"] = np.array([float(margins.get(k, np.inf)) for k in ("norm_u-u_max", "box centre plane", "normV")])
            print("%s, %s map: n = %d, max|J| = %.6g, dev_ref = %.3e, margins %s" % (name, tag, len(z), vx.amax(J), out[key + "dev_ref"],
                                                                                  out[key + "margins"].tolist()))
        starts = vx.newton_starts(z, NEWTON_FACTOR)
        res = vx.newton_rows(P, shipped, prob, starts)
        assert np.all(res["status"] == 1), res["status"]
        out[name + "_newton_starts"], out[name + "_newton_z"] = starts, res["z"]
        out[name + "_newton_rnorm"], out[name + "_newton_iters"] = res["rnorm"], res["iters"]
        print("%s: Newton from %d starts, iterations %s, max rnorm %.3e" % (name, len(starts), res["iters"].tolist(), res["rnorm"].max()))
    path = os.path.join(HERE, "vtol_exact_pin.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
