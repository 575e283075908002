#!/usr/bin/env python3
"""Generate the vtolUAV fixtures under tests/golden/ from the REFERENCE ITSELF.

Authoring container only (needs the reference tree; SOCP_REFERENCE names it).  In a temporary directory OUTSIDE
the repository it compiles

  (a) tests/golden/vtol_ref_driver.cpp with the reference's vtolUAV.cpp / obstacle.cpp / odeTools.cpp: the
      reference's own objects evaluated at given points;
  (b) tests/cpp/vtol_flow.cpp -DSOCP_REFERENCE_BUILD with the reference's shooting.cpp, odeTools.cpp, vtolUAV.cpp,
      obstacle.cpp and this repository's host hybrd (socp_amd/csrc/minpack.cpp),

each twice: with the flags of oracle/Makefile's REFFLAGS (-ffp-contract=off), and with -mfma -ffp-contract=fast --
the reference against itself under a rounding-level perturbation of every multiply-add, which is the yardstick of the
GPU tests' bars.  Only numbers are written: vtol_vectors.npz, vtol_rows.npz, vtol_flow.npz.

    python tests/golden/make_vtol_golden.py
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SOCP_REFERENCE", "/root/reference")
DATA = os.path.join(HERE, "vtol")

# SOCP_VTOL_NPARAMS order: u_max a_max alphaT alphaV invSigmaXwp Vd ca nWP_tot nWP | phiObs psiWP muObs sigmaWP
DEFAULTS = np.array([10, 0.3, 0.05, 0.0, 1.0 / 60, 1, 0.0, 0, 0, 1, 0.03, 1, 2.5])
I_UMAX, I_CA, I_NWP_TOT, I_NWP, I_MU = 0, 6, 7, 8, 11
MUS = (1.0, 0.3, 0.05)
CAS = (0.05, 0.0)
UMAXS = (1.0, 10.0)
STORED_STAGES = ("path_1", "ca", "path_2", "path_4", "path_8", "path_16", "path_32", "invSigma", "muObs", "u_max")
STORED_STAGES_8 = ("path_8", "u_max")
# stages that start from the solution of the stage before them: their z0 is that stage's z (asserted), not stored twice
Z0_FROM = {"ca": "path_1", "invSigma": "path_32", "muObs": "invSigma", "u_max": "muObs"}


def have_reference():
    return os.path.isfile(os.path.join(REF, "src", "models", "vtolUAV", "vtolUAV.cpp"))


def read_obstacles(path):
    """The obstacle file as the table socp_ctx_set_map takes: rows (type, centre xyz, radii xyz).  float() and the
    reference's `istream >> double` are both correctly rounded conversions."""
    rows = [ln.split() for ln in open(path).read().splitlines()]
    n = int(rows[1][0])
    typ = [float(rows[3 + i][0]) for i in range(n)]
    pos = [[float(v) for v in rows[4 + n + i][:3]] for i in range(n)]
    rad = [[float(v) for v in rows[5 + 2 * n + i][:3]] for i in range(n)]
    return np.array([[typ[i]] + pos[i] + rad[i] for i in range(n)])


def config_of(i):
    """Parameter block of point i: muObs, ca and u_max cycle through their values so that every combination occurs."""
    p = DEFAULTS.copy()
    p[I_MU] = MUS[i % 3]
    p[I_CA] = CAS[(i // 3) % 2]
    p[I_UMAX] = UMAXS[(i // 6) % 2]
    return p


def random_points(rng, table, n):
    lo = (table[:, 1:4] - table[:, 4:7]).min(axis=0) - 20
    hi = (table[:, 1:4] + table[:, 4:7]).max(axis=0) + 20
    X = np.zeros((n, 12))
    X[:, 0:3] = np.round(rng.uniform(lo, hi, (n, 3)) * 64) / 64
    direction = rng.normal(size=(n, 3))
    direction /= np.linalg.norm(direction, axis=1)[:, None]
    speed = np.exp(rng.uniform(np.log(1e-3), np.log(3.0), n))
    X[:, 3:6] = direction * speed[:, None]
    X[:, 6:9] = rng.uniform(-1, 1, (n, 3))
    # |p_v| / a_max is the unsaturated control norm: uniform on [0, 1.5] saturates a third of the points at u_max = 1, none at 10
    direction = rng.normal(size=(n, 3))
    direction /= np.linalg.norm(direction, axis=1)[:, None]
    X[:, 9:12] = direction * rng.uniform(0, 0.45, n)[:, None]
    X[:, 3:12] = np.round(X[:, 3:12] * 2.0 ** 26) / 2.0 ** 26        # short mantissas: the file compresses
    X[:, 3:6] = np.where(np.linalg.norm(X[:, 3:6], axis=1)[:, None] < 1e-3, X[:, 3:6] * 1.01, X[:, 3:6])
    return X


def extreme_points():
    """Hand-placed positions on the shipped map: a box face, centre planes (0/0 in the gradient, then the reset of the whole
    component), a box centre, and far outside (|h| up to ~4000 at muObs = 0.05).  Each at muObs = 1 and 0.05."""
    pos = [(11.5, 30, 10), (7.5, 30, 10), (30, 49, 10), (30, 30, 20), (200, 200, 150), (-95, -50, -80), (48, 73, 26), (35, 17.5, 20)]
    X, P = [], []
    for mu in (1.0, 0.05):
        for q in pos:
            X.append(list(q) + [0.4, -0.3, 0.1, 0.2, -0.1, 0.05, 0.06, -0.02, 0.03])
            p = DEFAULTS.copy()
            p[I_MU] = mu
            p[I_CA] = 0.05
            P.append(p)
    return np.array(X, dtype=float), np.array(P)


def near_surface_candidates(tables):
    """Positions within half a muObs of the surface of every box and ellipsoid of BOTH maps, at each muObs: where the penalty and
    its gradient are O(1/muObs) rather than vanishing -- the random points seldom land there, and the ellipsoid branch (type 0) is
    reachable through the synthetic map only.  A box gets one candidate per x / y face: the shipped boxes abut each other, and
    beside a shared face the two gradients cancel; near_surface_points keeps, per obstacle and muObs, the candidate where the
    reference's own gradient is largest.  Returns (map name, group, position, muObs) tuples."""
    cands = []
    along = np.array([0.6, 0.64, 0.48])                      # a unit direction with no zero component
    for name, table in tables.items():
        for o, row in enumerate(table):
            typ, c, r = row[0], row[1:4], row[4:7]
            if typ not in (0, 1):
                continue
            for k, mu in enumerate(MUS):
                side = 0.5 * mu if k % 2 == 0 else -0.5 * mu
                if typ == 1:      # beside a face, well inside the other two slabs
                    for axis, sign in ((0, 1), (0, -1), (1, 1), (1, -1)):
                        off = np.array([0.3 * r[0], 0.3 * r[1], -0.4 * r[2]])
                        off[axis] = sign * (r[axis] + side)
                        cands.append((name, (name, o, k), c + off, mu))
                else:             # along `along`, at the ellipsoid's radius in that direction
                    cands.append((name, (name, o, k), c + along * (1.0 / np.sqrt(np.sum(along ** 2 / r ** 2)) + side), mu))
    return cands


def near_surface_points(exes, tables, files):
    best = {}
    for name in tables:
        d = Driver(exes["driver_off"], os.path.join(DATA, files[name]), os.path.join(DATA, "waypoints"))
        for cname, group, q, mu in near_surface_candidates(tables):
            if cname != name:
                continue
            p = DEFAULTS.copy()
            p[I_MU] = mu
            p[I_CA] = 0.05
            d.ask("P", p)
            size = np.abs(d.ask("M", q)[1:4]).max()
            if group not in best or size > best[group][0]:
                best[group] = (size, q, p)
        d.close()
    X = [list(q) + [0.5, 0.2, -0.1, 0.3, -0.2, 0.1, 0.05, 0.04, -0.03] for _, q, _ in best.values()]
    return np.array(X), np.array([p for _, _, p in best.values()])


class Driver:
    def __init__(self, exe, obstacles, waypoints):
        self.p = subprocess.Popen([exe, obstacles, waypoints], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def ask(self, code, *arrays):
        vals = np.concatenate([np.atleast_1d(np.asarray(a, dtype=float)).ravel() for a in arrays]) if arrays else []
        self.p.stdin.write(code + " " + " ".join("%.17g" % v for v in vals) + "\n")
        self.p.stdin.flush()
        if code == "P":
            return None
        return np.array([float(v) for v in self.p.stdout.readline().split()])

    def close(self):
        self.p.stdin.close()
        self.p.wait()


def compile_all(tmp):
    src = os.path.join(REF, "src")
    model_srcs = [os.path.join(src, "socp", "odeTools.cpp"), os.path.join(src, "models", "vtolUAV", "vtolUAV.cpp"),
                  os.path.join(src, "maps", "obstacle", "obstacle.cpp")]
    flavours = {"off": ["-ffp-contract=off"], "fma": ["-mfma", "-ffp-contract=fast"]}
    exes = {}
    for tag, flags in flavours.items():
        common = ["g++", "-O2", "-std=gnu++11", "-w"] + flags + ["-I" + os.path.join(ROOT, "include"), "-I" + src,
                                                                    "-I" + os.path.join(ROOT, "socp_amd", "csrc")]
        exes["driver_" + tag] = os.path.join(tmp, "driver_" + tag)
        subprocess.check_call(common + ["-o", exes["driver_" + tag], os.path.join(HERE, "vtol_ref_driver.cpp")] + model_srcs)
        exes["flow_" + tag] = os.path.join(tmp, "flow_" + tag)
        subprocess.check_call(common + ["-DSOCP_REFERENCE_BUILD", "-o", exes["flow_" + tag], os.path.join(ROOT, "tests", "cpp", "vtol_flow.cpp"),
                                        os.path.join(src, "socp", "shooting.cpp")] + model_srcs +
                              [os.path.join(ROOT, "socp_amd", "csrc", "minpack.cpp"), "-lpthread"])
    return exes


def rel_dev(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(a)))) if a.size else 0.0


def make_vectors(exes):
    out, rows = {}, {}
    rng = np.random.default_rng(20261016)
    tables = {"shipped": read_obstacles(os.path.join(DATA, "obstacles")), "synthetic": read_obstacles(os.path.join(DATA, "obstacles_synthetic"))}
    files = {"shipped": "obstacles", "synthetic": "obstacles_synthetic"}
    n = 256
    X = random_points(rng, tables["shipped"], n)
    P = np.stack([config_of(i) for i in range(n)])
    Xe, Pe = extreme_points()
    out["X"], out["params"], out["ext_X"], out["ext_params"] = X, P, Xe, Pe
    Xn, Pn = near_surface_points(exes, tables, files)
    out["near_X"], out["near_params"] = Xn, Pn
    for name in ("shipped", "synthetic"):
        d = Driver(exes["driver_off"], os.path.join(DATA, files[name]), os.path.join(DATA, "waypoints"))
        out["table_" + name] = tables[name]
        if name == "shipped":
            w = d.ask("W")
            out["path"] = w[1:].reshape(int(w[0]), 6)

        def evaluate(Xs, Ps):
            res = []
            for x, p in zip(Xs, Ps):
                d.ask("P", p)
                res.append(d.ask("E", x))
            return np.stack(res)          # rhs 0:12, control 12:15, H 15, map Function 16, map Gradient 17:20
        E = evaluate(X, P)
        assert np.array_equal(E[:, 0:3], X[:, 3:6]) and np.array_equal(E[:, 6:9], 0 - E[:, 17:20])
        if name == "shipped":
            # rows 0..2 of the right-hand side are the velocity itself and rows 6..8 are 0 - Gradient (asserted above): not stored
            out["rhs_3_12"], out["ctl"] = E[:, 3:12], E[:, 12:15]
            Ee = evaluate(Xe, Pe)
            out["ext_rhs"], out["ext_ctl"], out["ext_ham"], out["ext_func"] = Ee[:, 0:12], Ee[:, 12:15], Ee[:, 15], Ee[:, 16]
            sat = np.linalg.norm(X[:, 9:12], axis=1) / 0.3
            print("saturated at u_max = 1: %d of %d; at 10: %d" % ((sat[P[:, I_UMAX] == 1] > 1).sum(), (P[:, I_UMAX] == 1).sum(), (sat > 10).sum()))
        else:
            out["syn_rhs_6_9"] = E[:, 6:9]      # the other rows do not read the map
        En = evaluate(Xn, Pn)
        pre = "near_" if name == "shipped" else "near_syn_"
        out[pre + "rhs_6_9"], out[pre + "ham"], out[pre + "func"] = En[:, 6:9], En[:, 15], En[:, 16]
        if name == "shipped":
            out["near_rhs_plain"], out["near_ctl"] = En[:, [0, 1, 2, 3, 4, 5, 9, 10, 11]], En[:, 12:15]
        print("%s map, near-surface points: %d with a gradient component above 1e-3" % (name, (np.abs(En[:, 6:9]).max(axis=1) > 1e-3).sum()))
        out[("" if name == "shipped" else "syn_") + "ham"] = E[:, 15]
        out[("" if name == "shipped" else "syn_") + "func"] = E[:, 16]
        d.close()

    # ---- one 100-step ModelInt segment from the first 64 points, both builds of the reference ----
    ns = 64
    t0 = np.round(rng.uniform(0, 5, ns) * 64) / 64
    tf = t0 + np.round(rng.uniform(0.5, 6, ns) * 64) / 64
    seg = {}
    for tag in ("off", "fma"):
        d = Driver(exes["driver_" + tag], os.path.join(DATA, "obstacles"), os.path.join(DATA, "waypoints"))
        res = []
        for i in range(ns):
            d.ask("P", P[i])
            res.append(d.ask("I", t0[i], tf[i], X[i]))
        seg[tag] = np.stack(res)
        d.close()
    rows["seg_t0"], rows["seg_tf"], rows["seg_Xf"] = t0, tf, seg["off"]
    rows["seg_self_dev"] = np.array(rel_dev(seg["off"], seg["fma"]))

    # ---- boundary rows for 16 mode patterns ----
    d = Driver(exes["driver_off"], os.path.join(DATA, "obstacles"), os.path.join(DATA, "waypoints"))
    nr = 16
    modes = rng.integers(0, 3, (nr, 6))
    modes[0], modes[1] = 0, 1
    Xr, Xpr = rng.uniform(-2, 2, (nr, 12)), rng.uniform(-2, 2, (nr, 12))
    Xr[:, 0:3] += 40
    Xpr[:, 0:3] += 40
    Xdr = Xr[:, 0:6] + rng.uniform(-1, 1, (nr, 6))
    Pr = np.tile(DEFAULTS, (nr, 1))
    Pr[:, I_NWP_TOT] = 32
    Pr[:, I_NWP] = np.arange(nr) * 2
    fin, sws = [], []
    for i in range(nr):
        d.ask("P", Pr[i])
        fin.append(d.ask("F", modes[i], Xr[i], Xdr[i]))
        sws.append(d.ask("S", Xr[i], Xpr[i], Xdr[i]))
    d.close()
    fin = np.stack(fin)
    rows.update(row_modes=modes.astype(np.int32), row_X=Xr, row_Xp=Xpr, row_Xd=Xdr, row_params=Pr,
                row_final=fin[:, 0:6], row_finalh=fin[:, 6:13], row_switching=np.stack(sws))
    return out, rows


def run_flow(exe, args, env_extra, timed=False):
    env = dict(os.environ, SOCP_VTOL_DATA=DATA, **env_extra)
    t_wall, t_cpu = time.time(), os.times()
    txt = subprocess.run([exe] + [str(a) for a in args], env=env, stdout=subprocess.PIPE, text=True, check=True).stdout
    t_cpu2 = os.times()
    recs = [json.loads(ln) for ln in txt.splitlines() if ln.startswith("{")]
    times = (time.time() - t_wall, (t_cpu2.children_user + t_cpu2.children_system) - (t_cpu.children_user + t_cpu.children_system))
    return (recs, times) if timed else recs


def pack_flow(out, prefix, recs, stored):
    stages = [r for r in recs if "stage" in r]
    out[prefix + "names"] = np.array([r["stage"] for r in stages])
    out[prefix + "info"] = np.array([r["info"] for r in stages], dtype=np.int32)
    out[prefix + "nfev"] = np.array([r["nfev"] for r in stages], dtype=np.int32)
    out[prefix + "n"] = np.array([r["n"] for r in stages], dtype=np.int32)
    for r in recs:
        name = r.get("stage", r.get("pre"))
        if name not in stored:
            continue
        if "stage" in r:
            out[prefix + name + "_z"] = np.array(r["z"])
        else:
            for key in ("z0", "F0", "time", "xd", "params"):
                out[prefix + name + "_" + key] = np.array(r[key])
            if name in Z0_FROM:
                if prefix == "":
                    assert np.array_equal(out[name + "_z0"], out[Z0_FROM[name] + "_z"])
                del out[prefix + name + "_z0"]
            out[prefix + name + "_mode_t"] = np.array(r["mode_t"], dtype=np.int8)
            out[prefix + name + "_mode_X"] = np.array(r["mode_X"], dtype=np.int8)


def make_flow(exes, tmp):
    out = {}
    zdir = {}
    for key in ("full", "cut"):
        zdir[key] = os.path.join(tmp, "z0_" + key)
        os.makedirs(zdir[key])
    cases = {"full": ([1e-10, 0, 60, 1], "", STORED_STAGES), "cut": ([1e-10, 0, 60, 1, 8], "wp8_", STORED_STAGES_8)}
    for key, (args, prefix, stored) in cases.items():
        # the unperturbed build first: it writes the z0 of every stage; the perturbed build then reports ITS F at the same z0
        pre = {"SOCP_FLOW_PRE": "1", "SOCP_FLOW_Z0_DIR": zdir[key]}
        recs, times = run_flow(exes["flow_off"], args, pre, timed=True)
        pert = run_flow(exes["flow_fma"], args, pre)
        pack_flow(out, prefix, recs, stored)
        dz, dF = [], []
        for name in stored:
            za = [r["z"] for r in recs if r.get("stage") == name][0]
            zb = [r["z"] for r in pert if r.get("stage") == name][0]
            Fa = [r["F0"] for r in recs if r.get("pre") == name][0]
            Fb = [r["F0"] for r in pert if r.get("pre") == name][0]
            dz.append(rel_dev(za, zb))
            dF.append(rel_dev(Fa, Fb))
        out[prefix + "stored"] = np.array(stored)
        out[prefix + "self_dev_z"] = np.array(dz)
        out[prefix + "self_dev_F0"] = np.array(dF)
        assert all(r["info"] == 1 for r in pert if "stage" in r), "the perturbed build of the reference did not converge"
        if key == "full":
            out["ref_wall_s"], out["ref_cpu_s"] = np.array(times[0]), np.array(times[1])
            model = [ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")]
            out["ref_machine"] = np.array("%s; %d residual threads; pre-solve reports included" % (model[0] if model else "unknown CPU", 4))
        # the program's own precision: info / nfev / final z only
        loose = [r for r in run_flow(exes["flow_off"], [1e-4] + args[1:], {}) if "stage" in r]
        out[prefix + "xtol4_info"] = np.array([r["info"] for r in loose], dtype=np.int32)
        out[prefix + "xtol4_nfev"] = np.array([r["nfev"] for r in loose], dtype=np.int32)
        out[prefix + "xtol4_z_final"] = np.array(loose[-1]["z"])
    # the map's own scalar moved THROUGH the program's real& (muObs 1 -> 0.5; the corner (60, 0.5) of the 8-waypoint case)
    moved = [r for r in run_flow(exes["flow_off"], [1e-10, 0, 60, 0.5, 8], {}) if "stage" in r]
    assert all(r["info"] == 1 for r in moved)
    out["wp8_mu05_nfev"] = np.array([r["nfev"] for r in moved], dtype=np.int32)
    out["wp8_mu05_muObs_z"] = np.array([r["z"] for r in moved if r["stage"] == "muObs"][0])
    out["wp8_mu05_u_max_z"] = np.array(moved[-1]["z"])
    assert rel_dev(out["wp8_mu05_muObs_z"], out["wp8_path_8_z"]) > 1e-3, "the continuation on muObs moved nothing"
    return out


def main():
    if not have_reference():
        print("reference tree %s not present: nothing generated (the committed fixtures stay as they are)" % REF)
        return 0
    tmp = tempfile.mkdtemp(prefix="vtol_golden_")
    try:
        exes = compile_all(tmp)
        vec, rows = make_vectors(exes)
        np.savez_compressed(os.path.join(HERE, "vtol_vectors.npz"), **vec)
        np.savez_compressed(os.path.join(HERE, "vtol_rows.npz"), **rows)
        flow = make_flow(exes, tmp)
        np.savez_compressed(os.path.join(HERE, "vtol_flow.npz"), **flow)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for f in ("vtol_vectors.npz", "vtol_rows.npz", "vtol_flow.npz"):
        print("%s: %d bytes" % (f, os.path.getsize(os.path.join(HERE, f))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
