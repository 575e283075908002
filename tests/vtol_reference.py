"""High-precision values and derived rounding bounds for the vtolUAV right-hand side, control and Hamiltonian with their obstacle
map (helper of test_vtol_pin_cpu.py, test_gpu_vtol_pin.py and golden/make_vtol_pin_golden.py, not a test).  The kits, the error
model and the decidability rule are those of fast_reference.py; this module restates the model once over the kit interface:

  vtol_ref   the reference operation order, expression by expression as VtolT<false> writes it (socp_amd/csrc/models_vtol.hpp:
             control_only, map_exact<F>, map_exact<G>, rhs, hamiltonian), with the upstream quirks: the ellipsoid gradient's `rad`
             without its z term, g2 = g2 - 0, the NaN reset of a whole component, phi*g + psi*0.0;
  vtol_fast  the structure of VtolT<true>: axis() with one exp per box axis, one shared reciprocal per box, the `pos` selection,
             the explicit NaN sign, rsqrt / rcp for the ellipsoid, the rsqrt-based rows 3-5 and 9-11.

Budgets: rcp and rsqrt C_RCP = C_RSQ = 2 (the constructions of the Goddard flavour); tanh and exp are the device library's, charged
C_TANH = 10 and C_EXP_LIB = 6 (fast_reference.py says where these come from).  Products carry their second-order term ea eb here
(fast_reference.second_order_products): far from a box in two or three axes every factor of the reference order's
(1 - tanh^2 hx)(1 - tanh hy)(1 - tanh hz) is an exact zero known to 10u, so the first-order terms vanish and ea eb is the bound --
of the order 1e-30 for two such factors, 1e-45 for three, where the value is 1e-60 or less.

NaN: no kit computes one.  Where the double arithmetic of either flavour produces a NaN the cause is an exact coincidence of inputs
(a position on a box's centre plane: dx == 0; on an ellipsoid's axis: hx == hy == 0; at its centre; a zero velocity), decided on the
inputs themselves.  A map component so poisoned is reset as a whole: value exactly 0, bound 0.  Rows 9-11 at zero velocity are NaN
(None here).

Decisions recorded as margins: norm_u > u_max (a real kink); h >= 0 per box axis / ellipsoid (`pos`: continuous, recorded all the
same); the sign selections dx > 0 / < 0 / == 0 compare input doubles (error zero, always decidable)."""
import numpy as np

import fast_reference as fr
from fast_reference import F64, C_EXP_LIB, F64Kit, MpfKit, TrackedKit, mpf

I_UMAX, I_AMAX, I_ALPHAT, I_ALPHAV, I_INVSIGMA, I_VD, I_CA, I_NWP_TOT, I_NWP, I_PHIOBS, I_PSIWP, I_MUOBS, I_SIGMAWP = range(13)
PLAIN = [0, 1, 2, 3, 4, 5, 9, 10, 11]                 # rows without the map (and so without tanh)
MAPPED = [6, 7, 8]
FAR_H = 20.0                                          # mutation "pos_far": the selection inverted where |h| exceeds this
FAR_BOX = 12.0                                        # mutation "g1_second_nearest_far": only a box at least this many muObs away


def _control(K, P, X):
    a_max, u_max = P[I_AMAX], P[I_UMAX]
    u = [-X[9] / a_max, -X[10] / a_max, -X[11] / a_max]
    norm_u = K.sqrt(u[0]*u[0] + u[1]*u[1] + u[2]*u[2])
    if K.cmp("norm_u-u_max", norm_u - u_max, ">"):
        u = [u[0] / norm_u*u_max, u[1] / norm_u*u_max, u[2] / norm_u*u_max]
    return u


def _zero(K, q):
    return K.value(q) == 0


def map_ref(K, P, tab, px, py, pz, want_f, want_g):
    """map_exact<WANT_F, WANT_G>: (func, [g0, g1, g2], reset[4] = which of f, g0, g1, g2 the NaN reset zeroed)."""
    mu = P[I_MUOBS]
    L = K.lift
    f, g0, g1, g2 = L(0.0), L(0.0), L(0.0), L(0.0)
    nan = [False] * 4
    for i, (typ, x, y, z, radx, rady, radz) in enumerate(tab):
        if typ == 0:
            hx, hy, hz = px - x, py - y, pz - z
            on_axis = K.cmp_exact("hx==0:%d" % i, px, x, "==") and K.cmp_exact("hy==0:%d" % i, py, y, "==")
            centre = on_axis and K.cmp_exact("hz==0:%d" % i, pz, z, "==")
            if want_f:
                if centre:
                    nan[0] = True                                                   # 0 / sqrt(0)
                else:
                    d = K.sqrt(hx*hx + hy*hy + hz*hz)
                    rad = d / K.sqrt(hx*hx / radx / radx + hy*hy / rady / rady + hz*hz / radz / radz)
                    h = (d - rad) / mu
                    f = f + (1 - K.tanh(h)) / 2
            if want_g:
                if on_axis:
                    nan[1] = nan[2] = True                                          # 0 * rho2, rho2 infinite or 0 / 0
                else:
                    d = K.sqrt(hx*hx + hy*hy + hz*hz)
                    q = K.sqrt(hx*hx / radx / radx + hy*hy / rady / rady)
                    rad = d / q
                    h = (d - rad) / mu
                    rho2 = (radx*radx - rady*rady) / (radx*radx*rady*rady) / q / q / q
                    th = K.tanh(h)
                    g0 = g0 - hx / d*(1 - hy*hy*rho2) / mu*(1 - th*th) / 2
                    g1 = g1 - hy / d*(1 + hx*hx*rho2) / mu*(1 - th*th) / 2
                g2 = g2 - 0
        elif typ == 1:
            dx, dy, dz = px - x, py - y, pz - z
            thx = K.tanh((abs(dx) - radx) / mu)
            thy = K.tanh((abs(dy) - rady) / mu)
            thz = K.tanh((abs(dz) - radz) / mu)
            if want_f:
                f = f + (1 - thx)*(1 - thy)*(1 - thz) / 8
            if want_g:
                if K.cmp_exact("dx==0:%d" % i, px, x, "=="):
                    nan[1] = True                                                   # 0 / |0|
                else:
                    g0 = g0 - dx / abs(dx) / mu*(1 - thx*thx)*(1 - thy)*(1 - thz) / 8
                if K.cmp_exact("dy==0:%d" % i, py, y, "=="):
                    nan[2] = True
                else:
                    g1 = g1 - dy / abs(dy) / mu*(1 - thy*thy)*(1 - thx)*(1 - thz) / 8
                if K.cmp_exact("dz==0:%d" % i, pz, z, "=="):
                    nan[3] = True
                else:
                    g2 = g2 - dz / abs(dz) / mu*(1 - thz*thz)*(1 - thx)*(1 - thy) / 8
    out = [L(0.0) if bad else q for bad, q in zip(nan, (f, g0, g1, g2))]
    phi, psi = P[I_PHIOBS], P[I_PSIWP]
    zero = L(0.0)
    return phi*out[0] + psi*zero, [phi*out[1] + psi*zero, phi*out[2] + psi*zero, phi*out[3] + psi*zero], nan


def _axis(K, name, h):
    pos = K.cmp(name, h, ">=")
    e = K.exp(-2.0 * abs(h))
    if getattr(K, "mutation", None) == "pos_far" and abs(K.value(h)) > FAR_H:
        pos = not pos
    return e, 1.0 + e, pos


def _second_nearest_box(K, tab, px, py, pz, beyond=None):
    """Index of the box second in the distance max(|dx| - radx, |dy| - rady, |dz| - radz), or -1; with `beyond`, -1 as well unless
    that distance exceeds it."""
    s = sorted((max(abs(K.value(px - x)) - K.value(radx), abs(K.value(py - y)) - K.value(rady), abs(K.value(pz - z)) - K.value(radz)), i)
               for i, (typ, x, y, z, radx, rady, radz) in enumerate(tab) if typ == 1)
    if len(s) < 2 or (beyond is not None and not s[1][0] > beyond):
        return -1
    return s[1][1]


def map_fast(K, P, tab, px, py, pz, want_f, want_g):
    """map_fast<WANT_F, WANT_G>."""
    mu = P[I_MUOBS]
    L = K.lift
    mutation = getattr(K, "mutation", None)
    flipped_box = -1
    if mutation == "g1_second_nearest":
        flipped_box = _second_nearest_box(K, tab, px, py, pz)
    elif mutation == "g1_second_nearest_far":
        flipped_box = _second_nearest_box(K, tab, px, py, pz, beyond=FAR_BOX * K.value(mu))
    inv_mu = K.rcp(mu)
    f, g0, g1, g2 = L(0.0), L(0.0), L(0.0), L(0.0)
    nan = [False] * 4
    for i, (typ, x, y, z, radx, rady, radz) in enumerate(tab):
        if typ == 0:
            hx, hy, hz = px - x, py - y, pz - z
            on_axis = K.cmp_exact("hx==0:%d" % i, px, x, "==") and K.cmp_exact("hy==0:%d" % i, py, y, "==")
            centre = on_axis and K.cmp_exact("hz==0:%d" % i, pz, z, "==")
            if centre:
                nan[0] = nan[1] = nan[2] = True                                     # rsqrt(0) is NaN
                continue
            d2 = hx*hx + hy*hy + hz*hz
            inv_d = K.rsqrt(d2)
            d = d2 * inv_d
            ax, ay, az = hx*hx*K.rcp(radx*radx), hy*hy*K.rcp(rady*rady), hz*hz*K.rcp(radz*radz)
            if want_f:
                h = (d - d * K.rsqrt(ax + ay + az)) * inv_mu
                e, w, pos = _axis(K, "h>=0:%d:f" % i, h)
                q = K.rcp(w)
                f = f + (e * q if pos else q)
            if want_g:
                if on_axis:
                    nan[1] = nan[2] = True
                    continue
                iq = K.rsqrt(ax + ay)
                h = (d - d * (K.rsqrt(ax + ay + az) if mutation == "zterm" else iq)) * inv_mu
                rho2 = (radx*radx - rady*rady) * K.rcp(radx*radx*rady*rady) * (iq*iq*iq)
                e, w, pos = _axis(K, "h>=0:%d:g" % i, h)
                q = K.rcp(w)
                s2 = 2.0 * e * q * q * inv_mu
                g0 = g0 - hx * inv_d * (1 - hy*hy*rho2) * s2
                g1 = g1 - hy * inv_d * (1 + hx*hx*rho2) * s2
        elif typ == 1:
            dx, dy, dz = px - x, py - y, pz - z
            ae, aw, apos = _axis(K, "h>=0:%d:x" % i, (abs(dx) - radx) * inv_mu)
            be, bw, bpos = _axis(K, "h>=0:%d:y" % i, (abs(dy) - rady) * inv_mu)
            ce, cw, cpos = _axis(K, "h>=0:%d:z" % i, (abs(dz) - radz) * inv_mu)
            bc = bw * cw
            r = K.rcp(aw * bc)
            qa, qb, qc = r * bc, r * (aw * cw), r * (aw * bw)
            ma, mb, mc = (ae * qa if apos else qa), (be * qb if bpos else qb), (ce * qc if cpos else qc)
            if want_f:
                f = f + ma * mb * mc
            if want_g:
                k = 2.0 * inv_mu
                tx, ty, tz = (k * ae * qa * qa) * (mb * mc), (k * be * qb * qb) * (ma * mc), (k * ce * qc * qc) * (ma * mb)
                if i == flipped_box:
                    ty = -ty
                # s * t with s = +-1 is exact: g - t or g + t
                if K.cmp_exact("dx==0:%d" % i, px, x, "=="):
                    nan[1] = True
                else:
                    g0 = g0 - tx if K.cmp_exact("dx>0:%d" % i, px, x, ">") else g0 + tx
                if K.cmp_exact("dy==0:%d" % i, py, y, "=="):
                    nan[2] = True
                else:
                    g1 = g1 - ty if K.cmp_exact("dy>0:%d" % i, py, y, ">") else g1 + ty
                if K.cmp_exact("dz==0:%d" % i, pz, z, "=="):
                    nan[3] = True
                else:
                    g2 = g2 - tz if K.cmp_exact("dz>0:%d" % i, pz, z, ">") else g2 + tz
    out = [L(0.0) if bad else q for bad, q in zip(nan, (f, g0, g1, g2))]
    phi = P[I_PHIOBS]
    return phi * out[0], [phi * out[1], phi * out[2], phi * out[3]], nan


def _still(K, X):
    return _zero(K, X[3]) and _zero(K, X[4]) and _zero(K, X[5])


def _hamiltonian(K, P, X, u, obs):
    """hamiltonian() of either flavour: the reference-order expression around the flavour's own map value."""
    vx, vy, vz, p_x, p_y, p_z, p_vx, p_vy, p_vz = X[3:12]
    a_max, ca, alphaV, Vd = P[I_AMAX], P[I_CA], P[I_ALPHAV], P[I_VD]
    normV = K.sqrt(vx*vx + vy*vy + vz*vz)
    norm_u = K.sqrt(u[0]*u[0] + u[1]*u[1] + u[2]*u[2])
    return (P[I_ALPHAT]*1
            + alphaV / 2*(normV - Vd)*(normV - Vd)
            + obs
            + a_max*a_max*norm_u*norm_u / 2
            + p_x*vx + p_y*vy + p_z*vz
            + (p_vx*(a_max*u[0] - ca*vx*normV) + p_vy*(a_max*u[1] - ca*vy*normV) + p_vz*(a_max*u[2] - ca*vz*normV)))


def vtol_ref(K, P, tab, X, want_h=True):
    """VtolT<false>.  Returns (Xdot[12] with None for a NaN component, u[3], H, reset[3] of rows 6-8)."""
    vx, vy, vz, p_x, p_y, p_z, p_vx, p_vy, p_vz = X[3:12]
    a_max, ca, alphaV, Vd = P[I_AMAX], P[I_CA], P[I_ALPHAV], P[I_VD]
    u = _control(K, P, X)
    _, g, nan = map_ref(K, P, tab, X[0], X[1], X[2], False, True)
    d = [None] * 12
    d[0], d[1], d[2] = vx, vy, vz
    d[6], d[7], d[8] = 0 - g[0], 0 - g[1], 0 - g[2]
    normV = K.sqrt(vx*vx + vy*vy + vz*vz)
    d[3] = a_max*u[0] - ca*vx*normV
    d[4] = a_max*u[1] - ca*vy*normV
    d[5] = a_max*u[2] - ca*vz*normV
    if not _still(K, X):                                                            # 0 / 0 otherwise
        d[9] = -p_x + ca*(p_vx*(normV + vx*vx / normV) + p_vy*(vy*vx / normV) + p_vz*(vz*vx / normV)) - alphaV*vx / normV*(normV - Vd)
        d[10] = -p_y + ca*(p_vy*(normV + vy*vy / normV) + p_vx*(vx*vy / normV) + p_vz*(vz*vy / normV)) - alphaV*vy / normV*(normV - Vd)
        d[11] = -p_z + ca*(p_vz*(normV + vz*vz / normV) + p_vx*(vx*vz / normV) + p_vy*(vy*vz / normV)) - alphaV*vz / normV*(normV - Vd)
    if not want_h:
        return d, u, None, nan[1:]
    obs = map_ref(K, P, tab, X[0], X[1], X[2], True, False)[0]
    return d, u, _hamiltonian(K, P, X, u, obs), nan[1:]


def vtol_fast(K, P, tab, X, want_h=True):
    """VtolT<true>.  Returns (Xdot[12], u[3], H, reset[3]); control and Hamiltonian are the reference-order expressions (compiled
    with contraction), the Hamiltonian around map_fast<F>."""
    vx, vy, vz, p_x, p_y, p_z, p_vx, p_vy, p_vz = X[3:12]
    a_max, ca, alphaV, Vd = P[I_AMAX], P[I_CA], P[I_ALPHAV], P[I_VD]
    mutation = getattr(K, "mutation", None)
    u = _control(K, P, X)
    _, g, nan = map_fast(K, P, tab, X[0], X[1], X[2], False, True)
    d = [None] * 12
    d[0], d[1], d[2] = vx, vy, vz
    d[6], d[7], d[8] = 0 - g[0], 0 - g[1], 0 - g[2]
    if _still(K, X):
        # rsqrt(0) is not finite: normV is v2 itself (zero) there, so rows 3-5 stay a_max u - 0 as upstream; rows 9-11 are NaN
        normV = K.lift(0.0)
        d[3] = a_max*u[0] - ca*vx*normV
        d[4] = a_max*u[1] - ca*vy*normV
        d[5] = a_max*u[2] - ca*vz*normV
    else:
        v2 = vx*vx + vy*vy + vz*vz
        inv = K.rsqrt(v2)
        normV = v2 * inv
        d[3] = a_max*u[0] - ca*vx*normV
        d[4] = a_max*u[1] - ca*vy*normV
        d[5] = a_max*u[2] - ca*vz*normV
        pv = (p_vx*vx + p_vy*vy + p_vz*vz) * inv
        w = alphaV * (normV - Vd) * inv
        if mutation == "w_sign":
            w = -w
        d[9] = -p_x + ca*(p_vx*normV + vx*pv) - w*vx
        d[10] = -p_y + ca*(p_vy*normV + vy*pv) - w*vy
        d[11] = -p_z + ca*(p_vz*normV + vz*pv) - w*vz
    if not want_h:
        return d, u, None, nan[1:]
    obs = map_fast(K, P, tab, X[0], X[1], X[2], True, False)[0]
    return d, u, _hamiltonian(K, P, X, u, obs), nan[1:]


# ---- running the restatements -----------------------------------------------------------------------------------------------

def lift_table(K, table):
    return [(float(r[0]),) + tuple(K.lift(v) for v in r[1:7]) for r in np.asarray(table, dtype=float).reshape(-1, 7)]


def run(fn, K, P, table, X):
    """fn on the kit's numbers; everything arrives as doubles."""
    with np.errstate(all="ignore"):
        return fn(K, [K.lift(p) for p in P], lift_table(K, table), [K.lift(q) for q in X])


def emulate(fn, P, table, X, **kit):
    """fn in numpy.float64, one rounding per operation: (Xdot[12] with NaN where the restatement says so, u[3], H)."""
    d, u, H, _ = run(fn, F64Kit(**kit), P, table, X)
    return np.array([np.nan if q is None else q for q in d], dtype=F64), np.array(u, dtype=F64), F64(H)


def _pin(tracked):
    """fast_reference._pin, with None -> (NaN, 0) and an untouched zero (the reset, free space) -> (0, 0)."""
    live = [fr.Tracked(0.0) if q is None else q for q in tracked]
    val, bnd = fr._pin(live)
    for k, q in enumerate(tracked):
        if q is None:
            val[k] = np.nan
    return val, bnd


def evaluate_row(P, table, X, flip=()):
    """One row through both restatements on Tracked numbers: value[12], B_ref[12], B_fast[12], u[3], B_u[3], H, B_H (reference
    order), B_H_fast (the same expression around map_fast<F>), reset[3] (rows 6-8 zeroed by the NaN reset), decidable, undecided."""
    Kr, Kf = TrackedKit(flip), TrackedKit(flip, c_exp=C_EXP_LIB)
    # far from a box every factor of the reference order's (1 - tanh^2 hx)(1 - tanh hy)(1 - tanh hz) is an exact zero with an error
    # of 10u: first order drops the whole product, the ea eb terms are what bounds it
    with fr.second_order_products():
        d_ref, u_ref, H_ref, reset = run(vtol_ref, Kr, P, table, X)
        d_fast, u_fast, H_fast, reset_fast = run(vtol_fast, Kf, P, table, X)
    assert reset == reset_fast and [q is None for q in d_ref] == [q is None for q in d_fast]
    # The VALUE is the throughput form's: 1 - tanh h and 1 - tanh^2 h as the reference order writes them cancel, and past |h| ~ 80
    # even 240 bits hold nothing of the difference, whereas e q and e q^2 are exact to the working precision at any h.  The
    # reference-order evaluation is the same function, so the two agree to an ABSOLUTE 2^-200 of the map's scale (asserted, unless
    # a decision is flipped: `pos` exists in one form only); B_ref carries the distance between them.
    scale = mpf(2) ** -200 * (1 + abs(Kr.lift(P[I_PHIOBS]).v / Kr.lift(P[I_MUOBS]).v) * (1 + len(lift_table(Kr, table))))
    pairs = [(a, b) for a, b in zip(d_ref + [H_ref], d_fast + [H_fast]) if a is not None]
    assert flip or all(abs(a.v - b.v) <= scale * (1 + abs(b.v)) for a, b in pairs), "the two restatements disagree"
    rebased = lambda a, b: None if a is None else fr.Tracked(b.v, a.e + abs(a.v - b.v))
    out = {"reset": np.array(reset)}
    out["value"], out["B_fast"] = _pin(d_fast)
    out["B_ref"] = _pin([rebased(a, b) for a, b in zip(d_ref, d_fast)])[1]
    out["u"], out["B_u"] = _pin(u_ref)
    h, out_bhf = _pin([H_fast])
    out["H"], out["B_H_fast"] = h[0], out_bhf[0]
    out["B_H"] = _pin([rebased(H_ref, H_fast)])[1][0]
    out["undecided"] = sorted(set(Kr.undecided()) | set(Kf.undecided()))
    out["decidable"] = not out["undecided"]
    return out


def value_mpf(P, tab, X):
    """The mathematical right-hand side on mpf numbers (P, tab, X already mpf)."""
    return vtol_ref(MpfKit(), P, tab, X, want_h=False)[0]


def rk4_mpf(P, table, X0, step, nsteps):
    """nsteps classical RK4 steps of size `step` (a double) in mpf (the right-hand side is autonomous)."""
    K = MpfKit()
    Pm, tab = [K.lift(p) for p in P], lift_table(K, table)
    h = mpf(float(step))
    X = [mpf(float(q)) for q in X0]
    f = lambda Y: value_mpf(Pm, tab, Y)
    for _ in range(nsteps):
        F1 = f(X)
        F2 = f([a + h / 2 * k for a, k in zip(X, F1)])
        F3 = f([a + h / 2 * k for a, k in zip(X, F2)])
        F4 = f([a + h * k for a, k in zip(X, F3)])
        X = [a + h / 6 * (k1 + (k4 + 2 * (k2 + k3))) for a, k1, k2, k3, k4 in zip(X, F1, F2, F3, F4)]
    return X
