#!/usr/bin/env python3
"""Writes tests/golden/vtol_pin.npz: the rows, 240-bit values and derived bounds that pin vtolUAV's right-hand side, control and
Hamiltonian in both flavours (tests/vtol_reference.py; read by tests/test_vtol_pin_cpu.py and tests/test_gpu_vtol_pin.py).

Authoring machine only: needs mpmath and the reference tree (SOCP_REFERENCE names it).  The reference's own double results for the
same rows (ref64_*) come from tests/golden/vtol_ref_driver.cpp, compiled with the reference's sources in a temporary directory
OUTSIDE the repository with the flags of oracle/Makefile's REFFLAGS, as make_vtol_golden.py does.  Only numbers are written.

    python tests/golden/make_vtol_pin_golden.py [out.npz]

Layout.  maps: table_<name> for MAPS; blocks: the parameter blocks.  Per row: map (index into map_names), block, group (index into
group_names), X, h_ray (single-obstacle rows: the nominal h of the sample, NaN elsewhere); val[9] = rows 3-11 of the right-hand side
at 240 bits rounded once to double (rows 0-2 are X[3:6] themselves), u[3], H; Bref[9], Bfast[9], Bu[3], BH, BHfast (BHfast: the
Hamiltonian around map_fast<F>); reset[3] (rows 6-8 zeroed as a whole by the NaN reset); dec; und (indices of the undecidable rows)
and alt_* (the same quantities on the other side of the undecided decisions); ref64_rhs[9], ref64_u[3], ref64_H.  Bounds are
rounded UP to 12 significant bits (at most 0.05 % wider; the file compresses).  traj_*: the segment data.

At least 95 % of the rows of every group but `kinks` must be decidable (asserted: a condition on the inputs).  The ray samples at
h = 0 sit on the surface itself, where the `pos` decision has margin zero: they are kept, with their h_ray, in the `kinks` group.

The ray's list of h is NOT complete on the inside: h < 0 is a depth of |h| muObs below the surface, and an obstacle is only so deep.
A sample that would lie at or beyond the centre (the box: dx <= 0; an ellipsoid: within 0.05 of it along the ray) does not exist
and is left out: at muObs = 1 everything from h = -40 on; at muObs = 0.05 from -300 on in the two ellipsoids and -4000 in the
box; at muObs = 1e-3 nothing.  155 of the 3 x 3 x 21 = 189 combinations remain; every h >= 0 is present at every muObs, and every
h < 0 at muObs = 1e-3."""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import fast_reference as fr                                   # noqa: E402
import vtol_reference as vr                                   # noqa: E402
import make_vtol_golden as mvg                                # noqa: E402

V = np.load(os.path.join(HERE, "vtol_vectors.npz"))
GROUPS = ["nominal", "parameters", "near_surface", "single_obstacle", "kinks", "grid256"]
MAPS = ["shipped", "synthetic", "box", "ellipsoid", "spheroid", "empty", "grid256"]
RAY_H = [0.0, 2.0 ** -30, 0.5, 5.0, 40.0, 300.0, 355.0, 365.0, 372.0, 400.0, 4000.0]
RAY_MU = [1.0, 0.05, 1e-3]
ALONG = np.array([0.6, 0.64, 0.48])
BOUND_BITS = 12
TRAJ_B, TRAJ_N, TRAJ_TF = 64, 100, 1.5625                     # step 2^-6: the hundred steps and their times are exact doubles
REGEN_ROWS = 12
SUB = list(range(3, 12))                                      # the stored rows of the right-hand side


def tables():
    grid = np.array([[1, 4 * i + 2, 4 * j + 2, 10, 1, 1, 5] for i in range(16) for j in range(16)], dtype=float)
    return {"shipped": V["table_shipped"], "synthetic": V["table_synthetic"],
            "box": np.array([[1, 30, 40, 20, 24, 9, 15]], dtype=float),
            "ellipsoid": np.array([[0, 30, 30, 12, 8, 5, 6]], dtype=float),
            "spheroid": np.array([[0, 30, 30, 12, 6, 6, 9]], dtype=float),
            "empty": np.zeros((0, 7)), "grid256": grid}


def block(**kw):
    p = mvg.DEFAULTS.copy()
    for k, v in kw.items():
        p[getattr(vr, "I_" + k.replace("_", "").upper())] = v
    return p


def parameter_blocks():
    """Eight blocks in which every listed value of every parameter occurs four times and every pair of values of two parameters at
    least once (a two-level orthogonal array), muObs and u_max cycling beside them."""
    lv = dict(alphaV=(0.05, 2.0), Vd=(1.0, 0.25), a_max=(0.3, 3.0), phiObs=(1.0, 40.0), alphaT=(0.05, 1.0), ca=(0.0, 0.05))
    out = []
    for k in range(8):
        a, b, c = k & 1, (k >> 1) & 1, (k >> 2) & 1
        bits = dict(alphaV=a, Vd=b, a_max=c, phiObs=a ^ b, alphaT=a ^ c, ca=b ^ c)
        out.append(block(muObs=mvg.MUS[k % 3], u_max=mvg.UMAXS[(k // 3) % 2], **{n: lv[n][bits[n]] for n in lv}))
    return out


def rows_all(T):
    rows = []

    def add(group, m, P, X, h=np.nan):
        rows.append(dict(group=group, map=m, P=np.array(P, dtype=float), X=np.array(X, dtype=float), h=h))

    for m in ("shipped", "synthetic"):
        for x, p in zip(V["X"], V["params"]):
            add("nominal", m, p, x)
    rng = np.random.default_rng(20261019)
    blocks = parameter_blocks()
    for m in ("shipped", "synthetic"):
        Xp = mvg.random_points(rng, T[m], 48)
        Xp[::6, 3:6] *= (1e-3 * 1.01 / np.linalg.norm(Xp[::6, 3:6], axis=1))[:, None]        # normV down to 1e-3
        for i, x in enumerate(Xp):
            add("parameters", m, blocks[i % 8], x)
    for m in ("shipped", "synthetic"):
        for x, p in zip(V["near_X"], V["near_params"]):
            add("near_surface", m, p, x)
    tail = [0.4, -0.3, 0.1, 0.2, -0.1, 0.05, 0.06, -0.02, 0.03]
    for m in ("box", "ellipsoid", "spheroid"):
        o = T[m][0]
        for mu in RAY_MU:
            for h in [s * q for q in RAY_H for s in ((1, -1) if q else (1,))]:
                if m == "box":
                    dx = o[4] + h * mu
                    pos = o[1:4] + np.array([dx, 0.3 * o[5], -0.4 * o[6]])
                    ok = dx > 0
                else:
                    t = 1.0 / np.sqrt(ALONG[0] ** 2 / o[4] ** 2 + ALONG[1] ** 2 / o[5] ** 2) + h * mu
                    pos = o[1:4] + ALONG * t
                    ok = t > 0.05
                if ok:                      # on the surface itself the `pos` decision is undecidable by construction: a kink row
                    add("single_obstacle" if h else "kinks", m, block(muObs=mu, ca=0.05, alphaV=0.05), list(pos) + tail, h)
    # kinks and resets
    direction = np.array([0.6, -0.64, 0.48])
    for k in (1, 10 ** 3, 10 ** 6):
        for s in (1, -1):
            x = V["X"][0].copy()
            x[9:12] = -direction * (0.3 * 1.0) * (1 + s * k * 2.0 ** -52)
            add("kinks", "shipped", block(u_max=1.0, ca=0.05, alphaV=0.05), x)
    b0, b7 = T["shipped"][0], T["shipped"][7]
    for mu in (1.0, 0.05):
        P = block(muObs=mu, ca=0.05, alphaV=0.05)
        for pos in ([b0[1] + b0[4], 30, 10], [b0[1] - b0[4], 30, 10], [30, b7[2] + b7[5], 30],        # box faces exactly
                    [b0[1], 30, 10], [30, b0[2], 10], [30, 30, 20],                                 # one centre plane
                    [b0[1], b0[2], 10], [b7[1], 60, b7[3]],                                         # two
                    [b0[1], b0[2], b0[3]], [b7[1], b7[2], b7[3]]):                                  # a box centre
            add("kinks", "shipped", P, pos + tail)
        for m in ("ellipsoid", "spheroid"):
            c = T[m][0][1:4]
            for pos in (c + [0, 0, 3], c - [0, 0, 7.5], c, c + [0, 2, 1]):                          # axis, axis, centre, hx == 0 alone
                add("kinks", m, P, list(pos) + tail)
        c = T["synthetic"][0][1:4]
        add("kinks", "synthetic", P, list(c + [0, 0, 2.5]) + tail)
        add("kinks", "synthetic", P, list(c) + tail)
    for ca, alphaV in ((0.05, 0.05), (0.0, 0.0), (0.05, 0.0)):                                      # normV = 0: rows 9-11 are NaN upstream
        x = V["X"][1].copy()
        x[3:6] = 0.0
        add("kinks", "shipped", block(ca=ca, alphaV=alphaV, muObs=0.3), x)
    add("kinks", "empty", block(ca=0.05, alphaV=0.05), V["X"][2])                                   # free space
    Xg = mvg.random_points(rng, T["grid256"], 32)
    Xg[:, 0:3] = np.round(rng.uniform([0, 0, 4], [64, 64, 16], (32, 3)) * 64) / 64 + 1.0 / 128      # inside, on no centre plane
    for i, x in enumerate(Xg):
        add("grid256", "grid256", block(muObs=mvg.MUS[i % 3], ca=0.05, alphaV=0.05), x)
    return rows


def round_up(b):
    """Bounds rounded up to BOUND_BITS significant bits (zero and subnormals untouched)."""
    b = np.asarray(b, dtype=float)
    m, e = np.frexp(b)
    r = np.ldexp(np.ceil(m * 2.0 ** BOUND_BITS) / 2.0 ** BOUND_BITS, e)
    return np.where((b == 0) | (b < 2.0 ** -1000), b, r)


KEYS = [("val", "value"), ("Bref", "B_ref"), ("Bfast", "B_fast"), ("u", "u"), ("Bu", "B_u"), ("H", "H"), ("BH", "B_H"), ("BHfast", "B_H_fast"),
        ("reset", "reset")]


def stored(e, key, src):
    q = np.asarray(e[src])
    if src in ("value", "B_ref", "B_fast"):
        q = q[SUB]
    return round_up(q) if key.startswith("B") else q


def reference_numbers(rows, T):
    """ref64: every row through the reference's own objects."""
    if not mvg.have_reference():
        raise SystemExit("reference tree %s not present" % mvg.REF)
    tmp = tempfile.mkdtemp(prefix="vtol_pin_golden_")
    out = np.empty((len(rows), 16))
    try:
        src = os.path.join(mvg.REF, "src")
        exe = os.path.join(tmp, "driver")
        subprocess.check_call(["g++", "-O2", "-std=gnu++11", "-w", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + src,
                               "-I" + os.path.join(ROOT, "socp_amd", "csrc"), "-o", exe, os.path.join(HERE, "vtol_ref_driver.cpp"),
                               os.path.join(src, "socp", "odeTools.cpp"), os.path.join(src, "models", "vtolUAV", "vtolUAV.cpp"),
                               os.path.join(src, "maps", "obstacle", "obstacle.cpp")])
        drivers = {}
        for name, tab in T.items():
            path = os.path.join(tmp, "obstacles_" + name)
            with open(path, "w") as f:
                f.write("n:\n\t%d\ntype:\n" % len(tab) + "".join("\t%d\n" % r[0] for r in tab) + "position:\n" +
                        "".join("\t%r\t%r\t%r\n" % tuple(float(v) for v in r[1:4]) for r in tab) + "radius:\n" +
                        "".join("\t%r\t%r\t%r\n" % tuple(float(v) for v in r[4:7]) for r in tab))
            drivers[name] = mvg.Driver(exe, path, os.path.join(mvg.DATA, "waypoints"))
        for i, r in enumerate(rows):
            d = drivers[r["map"]]
            d.ask("P", r["P"])
            out[i] = d.ask("E", r["X"])[:16]
        d = drivers["shipped"]
        d.ask("P", TRAJ_P)
        traj = np.stack([d.ask("I", 0.0, TRAJ_TF, x) for x in V["X"][:TRAJ_B]])
        for d in drivers.values():
            d.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return out, traj


TRAJ_P = block(muObs=0.3, ca=0.05, alphaV=0.05)


def regenerate(fix, idx):
    """Rows idx of the stored fixture evaluated afresh: [(stored, fresh)] arrays to compare bit for bit."""
    pairs = []
    for i in idx:
        e = vr.evaluate_row(fix["blocks"][fix["block"][i]], fix["table_" + str(fix["map_names"][fix["map"][i]])], fix["X"][i])
        for key, src in KEYS:
            pairs.append((fix[key][i], stored(e, key, src)))
        pairs.append((np.array(fix["dec"][i]), np.array(e["decidable"])))
    return pairs


def main(out_path):
    T = tables()
    rows = rows_all(T)
    blocks = []
    for r in rows:
        if not any(np.array_equal(r["P"], b) for b in blocks):
            blocks.append(r["P"])
    out = {"group_names": np.array(GROUPS), "map_names": np.array(MAPS), "blocks": np.array(blocks),
           "block": np.array([[np.array_equal(r["P"], b) for b in blocks].index(True) for r in rows], dtype=np.int16),
           "map": np.array([MAPS.index(r["map"]) for r in rows], dtype=np.int8),
           "group": np.array([GROUPS.index(r["group"]) for r in rows], dtype=np.int8),
           "X": np.array([r["X"] for r in rows]), "h_ray": np.array([r["h"] for r in rows])}
    for name, tab in T.items():
        out["table_" + name] = tab
    ev = [vr.evaluate_row(r["P"], T[r["map"]], r["X"]) for r in rows]
    for key, src in KEYS:
        out[key] = np.array([stored(e, key, src) for e in ev])
    out["dec"] = np.array([e["decidable"] for e in ev])
    und = [i for i, e in enumerate(ev) if not e["decidable"]]
    alt = [vr.evaluate_row(rows[i]["P"], T[rows[i]["map"]], rows[i]["X"], flip=ev[i]["undecided"]) for i in und]
    out["und"] = np.array(und, dtype=np.int32)
    for key, src in KEYS:
        out["alt_" + key] = np.array([stored(e, key, src) for e in alt]).reshape((len(und),) + out[key].shape[1:])
    for g, name in enumerate(GROUPS):
        sel = out["group"] == g
        share = out["dec"][sel].mean()
        print("%-16s %4d rows, decidable %.1f %%; undecided: %s" % (name, sel.sum(), 100 * share,
              sorted(set(n.split(":")[0] for i in np.flatnonzero(sel) for n in ev[i]["undecided"]))))
        assert name == "kinks" or share >= 0.95, "move the points of group " + name
    assert len(und), "no undecidable row left: the two-branch test would check nothing"
    E, traj = reference_numbers(rows, T)
    out["ref64_rhs"], out["ref64_u"], out["ref64_H"] = E[:, 3:12], E[:, 12:15], E[:, 15]
    assert all(np.array_equal(E[i, 0:3], rows[i]["X"][3:6]) for i in range(len(rows)))
    # the segment: the same recurrence in mpf on the mathematical right-hand side, and the reference's own deviation from it
    step = TRAJ_TF / TRAJ_N
    assert step == 2.0 ** -6 and step * TRAJ_N == TRAJ_TF
    X0 = V["X"][:TRAJ_B]
    ref = [vr.rk4_mpf(TRAJ_P, T["shipped"], x, step, TRAJ_N) for x in X0]
    dev = np.array([[fr._up(abs(fr.mpf(float(traj[b, c])) - ref[b][c])) for c in range(12)] for b in range(TRAJ_B)])
    out.update(traj_P=TRAJ_P, traj_X0=X0, traj_tf=np.array(TRAJ_TF), traj_N=np.array(TRAJ_N),
               traj_mpf=np.array([[float(q) for q in row] for row in ref]), traj_ref_dev=dev.max(axis=0))
    np.savez_compressed(out_path, **out)
    print("rows %d, undecidable %d, blocks %d; wrote %s, %d bytes" % (len(rows), len(und), len(blocks), out_path, os.path.getsize(out_path)))
    assert os.path.getsize(out_path) <= os.path.getsize(os.path.join(HERE, "fast_pin.npz"))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "vtol_pin.npz"))
